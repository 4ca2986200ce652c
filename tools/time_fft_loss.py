#!/usr/bin/env python3
"""Evidence for DESIGN 26 (the frequency-domain training loss), run on the MI355X box from the repo root:

  python tools/time_fft_loss.py                 every mode below, each as a child process under its own time limit; stops
                                                at the first child that does not exit normally
  python tools/time_fft_loss.py kernel          ops.fft_loss forward + backward (k_fft_diff, k_fft_rows, k_fft_cols,
                                                k_fft_grad, k_fft_final; the backward seeded with the unit seed: no further
                                                launch), called and as a replayed graph, and loss only, against the torch
                                                composition in fp32 on the same device (fft2 of both tensors, view_as_real,
                                                l1_loss, autograd), called
  python tools/time_fft_loss.py torch_replay    the torch composition captured into a graph and replayed, where it captures
  python tools/time_fft_loss.py step            one replayed EDSR x4 train step at c4's shape (128 LR patches of 32 x 32,
                                                Adam, L1) with --fft_weight 0 and 0.1
  python tools/time_fft_loss.py trace           ten plain calls at two shapes, for a kernel trace

Shapes: [128, 3, 128, 128] (c4's HR batch), [256, 1, 41, 41] (c3), [16, 3, 128, 128], [16, 3, 192, 192].
HIP events; medians over five alternating rounds of 30 timed calls (steps: 20) each, with the spread of the round medians."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((128, 3, 128, 128), (256, 1, 41, 41), (16, 3, 128, 128), (16, 3, 192, 192))
LIMITS = {"kernel": 420, "torch_replay": 240, "step": 420}


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


def _fmt(r):
    return "%8.3f ms (rounds %.3f .. %.3f)" % r


def torch_composition(x, y):
    """BasicSR's FFTLoss: nn.L1Loss()(view_as_real(fft2(pred)), view_as_real(fft2(target))), fp32."""
    import torch
    import torch.nn.functional as F
    return F.l1_loss(torch.view_as_real(torch.fft.fft2(x)), torch.view_as_real(torch.fft.fft2(y)))


def _pair(shape, dev, gen):
    import torch
    t = torch.rand(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    x = (t + 0.05 * torch.randn(shape, generator=gen).to(dev)).contiguous(memory_format=torch.channels_last)
    return x.requires_grad_(True), t


def kernel():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    for shape in SHAPES:
        x, t = _pair(shape, dev, gen)

        def fused():
            x.grad = None
            ops.backward(ops.fft_loss(x, t))

        def torch_side():
            x.grad = None
            torch_composition(x, t).backward()

        xd = x.detach()

        def forward_only():     # (a pred that needs no gradient: the loss-only launches)
            ops.fft_loss(xd, t)
        fused()
        a, ga = float(ops.fft_loss(x, t).detach()), x.grad.clone()
        torch_side()
        b, gb = float(torch_composition(x, t).detach()), x.grad.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused()
        r = _compare({"kernel": fused, "replayed": graph.replay, "torch": torch_side, "loss only": forward_only}, 30)
        m = shape[0] * shape[1] * shape[2] * shape[3]
        print("%-16s fft_loss fwd+bwd called %s, replayed %s, loss only %s | torch composition fwd+bwd called %s = %.2f x the "
              "replayed kernels | %.2f ns per value | loss %.7f vs %.7f, gradients differ by %.2e of their maximum"
              % ("x".join(str(v) for v in shape), _fmt(r["kernel"]), _fmt(r["replayed"]), _fmt(r["loss only"]), _fmt(r["torch"]),
                 r["torch"][0] / r["replayed"][0], r["replayed"][0] * 1e6 / m, a, b,
                 float((ga - gb).abs().max() / gb.abs().max())), flush=True)
        del x, t, ga, gb, graph
        torch.cuda.empty_cache()


def torch_replay():
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    for shape in SHAPES:
        x, t = _pair(shape, dev, gen)

        def torch_side():
            x.grad = None
            torch_composition(x, t).backward()
        for _ in range(3):
            torch_side()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                torch_side()
        except Exception as e:   # the library's plan may not be capturable
            print("%-16s the torch composition does not capture: %s" % ("x".join(str(v) for v in shape), str(e).splitlines()[0]), flush=True)
            return
        r = _compare({"replayed": graph.replay}, 30)
        print("%-16s torch composition fwd+bwd replayed %s" % ("x".join(str(v) for v in shape), _fmt(r["replayed"])), flush=True)
        del x, t, graph
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
    for w in (0.0, 0.1):
        net = pkg.EDSRNet(3, 64, 16)
        fill.fill_module(net, 3, 0.5)
        net.to(dev).train()
        flat, opt, dp, eager = pkg.trainers.build("edsr", net, 1e-5, fft_weight=w)
        g = pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat])
        steps[w] = (g, net, opt)
    r = _compare({w: (lambda s=s: s[0](*s[0].static)) for w, s in steps.items()}, 20)
    base, mix = r[0.0], r[0.1]
    print("EDSR x4 step, 128 x 3 x 32 x 32 -> 128 x 128, replayed graph: --fft_weight 0 %s | --fft_weight 0.1 %s | the loss "
          "adds %.3f ms = %.2f %%" % (_fmt(base), _fmt(mix), mix[0] - base[0], (mix[0] / base[0] - 1) * 100), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def trace():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    for shape in SHAPES[:2]:
        x, t = _pair(shape, dev, gen)
        for _ in range(10):
            x.grad = None
            ops.backward(ops.fft_loss(x, t))
        torch.cuda.synchronize()


def everything():
    for mode in ("kernel", "torch_replay", "step"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), mode], cwd=ROOT, timeout=LIMITS[mode]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("mode %s ended with status %d: nothing further is started" % (mode, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(everything())
    {"kernel": kernel, "torch_replay": torch_replay, "step": step, "trace": trace}[sys.argv[1]]()
