#!/usr/bin/env python3
"""Evidence for DESIGN 22 (the weight EMA fused into the optimizer kernels), run on the MI355X box from the repo root:

  python tools/time_ema.py kernel   one optimizer launch over a flat buffer, three ways: plain (srk_adam_step / srk_sgd_step),
                                    plain + a separate srk_axpby launch that updates the shadow (ema = d * ema + (1 - d) * p),
                                    and fused (srk_adam_step_ema / srk_sgd_step_ema) -- Adam at EDSR's 1.52 M parameters,
                                    SGD with Nesterov momentum at SRGAN-D's 38.2 M
  python tools/time_ema.py step     one replayed EDSR x4 train step at c4's shape (128 LR patches of 32 x 32, Adam, L1) with
                                    ema_decay 0 (the step as it is without the feature) and 0.999

HIP events; medians over five alternating rounds of 200 timed calls (steps: 20) each, with the spread of the round medians."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 0.999


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


def _params(pkg, make):
    """Length of the flat buffer FlatParams would give the model (every parameter padded to 16 bytes)."""
    return sum((p.numel() + 3) // 4 * 4 for p in make(pkg).parameters())


def kernel():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    cases = (("Adam, EDSR", "adam", _params(pkg, lambda m: m.EDSRNet(3, 64, 16)), 28, 36),
             ("SGD nesterov, SRGAN-D", "sgd", _params(pkg, lambda m: m.SRGANDiscriminator(3, 64, 128)), 20, 28))
    for name, kind, n, plain_bytes, fused_bytes in cases:
        p, g, m, v, e = [torch.randn(n, generator=gen).to(dev) * 0.01 for _ in range(5)]
        v.abs_()
        step = torch.zeros(2, dtype=torch.int32, device=dev)
        lr = torch.tensor([1e-5], device=dev)
        gs = torch.ones(1, device=dev)
        if kind == "adam":
            args = [ptr(p), ptr(g), ptr(m), ptr(v), n, 0.0, 0.9, 0.999, 1e-8, 0.0, ptr(step), ptr(lr), ptr(gs)]
            plain_fn, fused_fn = lib.srk_adam_step, lib.srk_adam_step_ema
        else:
            args = [ptr(p), ptr(g), ptr(m), n, 0.0, 0.9, 0.0, 1, 0, ptr(lr), ptr(gs)]
            plain_fn, fused_fn = lib.srk_sgd_step, lib.srk_sgd_step_ema

        def plain():
            check(plain_fn(*(args + [stream_ptr()])), "plain")

        def two_launches():
            plain()
            check(lib.srk_axpby(ptr(e), ptr(p), ptr(e), n, D, 1.0 - D, stream_ptr()), "srk_axpby")

        def fused():
            check(fused_fn(*(args + [ptr(e), D, stream_ptr()])), "fused")

        r = _compare({"plain": plain, "two": two_launches, "fused": fused}, 200)
        a, b, c = r["plain"], r["two"], r["fused"]
        print("%-22s %9d floats: plain %8.2f us (rounds %.2f .. %.2f) = %.2f TB/s of its %d B/param | plain + srk_axpby "
              "%8.2f us (rounds %.2f .. %.2f) | fused %8.2f us (rounds %.2f .. %.2f) = %.2f TB/s of its %d B/param | fused / "
              "plain %.3f (bytes: %.3f), fused / two launches %.3f"
              % (name, n, a[0] * 1e3, a[1] * 1e3, a[2] * 1e3, n * plain_bytes / (a[0] * 1e-3) / 1e12, plain_bytes,
                 b[0] * 1e3, b[1] * 1e3, b[2] * 1e3, c[0] * 1e3, c[1] * 1e3, c[2] * 1e3,
                 n * fused_bytes / (c[0] * 1e-3) / 1e12, fused_bytes, c[0] / a[0], fused_bytes / plain_bytes, c[0] / b[0]),
              flush=True)
        del p, g, m, v, e
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
    for d in (0.0, D):
        net = pkg.EDSRNet(3, 64, 16)
        fill.fill_module(net, 3, 0.5)
        net.to(dev).train()
        flat, opt, dp, eager = pkg.trainers.build("edsr", net, 1e-5, ema_decay=d)
        g = pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat])
        steps[d] = (g, net, opt)
    r = _compare({d: (lambda s=s: s[0](*s[0].static)) for d, s in steps.items()}, 20)
    base, ema = r[0.0], r[D]
    print("EDSR x4 step, 128 x 3 x 32 x 32 -> 128 x 128, replayed graph: ema_decay 0 %8.3f ms (rounds %.3f .. %.3f) | "
          "ema_decay %g %8.3f ms (rounds %.3f .. %.3f) | the EMA adds %.3f ms = %.2f %%"
          % (base[0], base[1], base[2], D, ema[0], ema[1], ema[2], ema[0] - base[0], (ema[0] / base[0] - 1) * 100), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


if __name__ == "__main__":
    {"kernel": kernel, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernel"]()
