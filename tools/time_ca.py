#!/usr/bin/env python3
"""Evidence for DESIGN 25 (channel attention, RCAN), run on the MI355X box from the repo root:

  python tools/time_ca.py op          ops.channel_attention, forward and forward + backward, against the torch composition
                                      on channels_last tensors (adaptive_avg_pool2d, two conv2d, relu, sigmoid, mul, add) at
                                      [16, 64, 48, 48] (the EDSR trainer's LR patch) and [128, 64, 32, 32]; with the
                                      fraction of the HBM roofline the fused op reaches; each figure twice: called from
                                      Python (allocations, ctypes, autograd: the host's time) and replayed from a captured
                                      graph (the device's time, as a trainer runs it)
  python tools/time_ca.py step 2 4    one replayed RCAN x4 train step (batch 16, 48 x 48 LR, Adam, L1) of 2 groups x 4
  python tools/time_ca.py step 10 20  blocks / of the paper's 10 x 20, with the fused op and with the composition in its place
  python tools/time_ca.py parity      the op against the fp64 restatement on the case table of the tests: worst error per
                                      output over max |ref| (the bars are 1e-4 for y, 1e-3 for gradients)
  python tools/time_ca.py all         each of the above as a child process under a time limit of its own, stopping at the
                                      first that fails

HIP events; medians over five alternating rounds of 30 timed calls (steps: 10) each, with the min and max of the round
medians.  Roofline: the op's algorithmic traffic is four passes of N*H*W*C*4 bytes each way (forward reads t twice and x
once and writes y; backward reads g twice and t once and writes dt) over 6.3 TB/s, the bandwidth a streaming kernel
reaches on this part."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((16, 64, 48, 48), (128, 64, 32, 32))
HBM_BYTES_PER_S = 6.3e12
CHILD_LIMITS = (("op", 180), ("parity", 120), ("step 2 4", 180), ("step 10 20", 420))


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
    return "%8.2f us (rounds %.2f .. %.2f)" % (1e3 * r[0], 1e3 * r[1], 1e3 * r[2])


def op():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import ca_ref
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    for shape in SHAPES:
        n, c, h, w = shape
        cl = lambda: torch.randn(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        t, x, g = cl().requires_grad_(True), cl().requires_grad_(True), cl()
        par = [(0.5 * torch.randn(s, generator=gen)).to(dev).requires_grad_(True)
               for s in ((c // 16, c, 1, 1), (c // 16,), (c, c // 16, 1, 1), (c,))]
        leaves = [t, x] + par

        def fused_fwd():
            with torch.no_grad():
                ops.channel_attention(t, x, *par)

        def torch_fwd():
            with torch.no_grad():
                ca_ref.composition(t, x, *par)

        def fused():
            torch.autograd.grad(ops.channel_attention(t, x, *par), leaves, g)

        def composed():
            torch.autograd.grad(ca_ref.composition(t, x, *par), leaves, g)

        a = torch.autograd.grad(ops.channel_attention(t, x, *par), leaves, g)
        b = torch.autograd.grad(ca_ref.composition(t, x, *par), leaves, g)
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        r = _compare({"fused fwd": fused_fwd, "torch fwd": torch_fwd, "fused": fused, "torch": composed}, 30)
        one_way = 4.0 * n * h * w * c * 4 / HBM_BYTES_PER_S * 1e3      # ms
        print("%-14s forward          fused %s | torch composition %s = %.2f x the fused op | roofline %.2f us: the fused op "
              "reaches %.0f %% of it" % ("x".join(map(str, shape)), _fmt(r["fused fwd"]), _fmt(r["torch fwd"]),
                                         r["torch fwd"][0] / r["fused fwd"][0], 1e3 * one_way,
                                         100 * one_way / r["fused fwd"][0]), flush=True)
        print("%-14s forward+backward fused %s | torch composition %s = %.2f x the fused op | roofline %.2f us: the fused op "
              "reaches %.0f %% of it | gradients of the two differ by %.1e of their maximum"
              % ("x".join(map(str, shape)), _fmt(r["fused"]), _fmt(r["torch"]), r["torch"][0] / r["fused"][0],
                 2e3 * one_way, 200 * one_way / r["fused"][0], diff), flush=True)
        # the same four calls replayed from a captured graph: the device's time without the host's per-call work, which is
        # how a trainer runs them
        graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in
                  (("fused fwd", fused_fwd), ("torch fwd", torch_fwd), ("fused", fused), ("torch", composed))}
        r = _compare(graphs, 30)
        print("%-14s replayed graph: forward fused %s | torch %s = %.2f x | %.0f %% of the roofline"
              % ("x".join(map(str, shape)), _fmt(r["fused fwd"]), _fmt(r["torch fwd"]), r["torch fwd"][0] / r["fused fwd"][0],
                 100 * one_way / r["fused fwd"][0]), flush=True)
        print("%-14s replayed graph: forward+backward fused %s | torch %s = %.2f x | %.0f %% of the roofline"
              % ("x".join(map(str, shape)), _fmt(r["fused"]), _fmt(r["torch"]), r["torch"][0] / r["fused"][0],
                 200 * one_way / r["fused"][0]), flush=True)
        for gr in graphs.values():
            gr.close()


class _Composed(object):
    """base_networks.ChannelAttention.forward with the torch composition in the op's place (the timing's other side)."""

    def __enter__(self):
        import ca_ref
        from pytorch_super_resolution_model_collection_amd import base_networks as B
        self.cls, self.old = B.ChannelAttention, B.ChannelAttention.forward

        def forward(m, t, residual=None, res_box=None):
            down, up = m.conv_du[0], m.conv_du[2]
            return ca_ref.composition(t, residual, down.weight, down.bias, up.weight, up.bias)
        B.ChannelAttention.forward = forward
        return self

    def __exit__(self, *a):
        self.cls.forward = self.old


def step(groups, blocks):
    import contextlib
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((16, 3, 48, 48), generator=gen).to(dev), torch.rand((16, 3, 192, 192), generator=gen).to(dev)
    steps = {}
    for side in ("fused", "composition"):
        with (_Composed() if side == "composition" else contextlib.nullcontext()):
            net = pkg.RCANNet(3, 64, groups, blocks, 16, 4)
            fill.fill_module(net, 3, 0.1)
            net.to(dev).train()
            flat, opt, dp, eager = pkg.trainers.build("rcan", net, 1e-5)
            steps[side] = (pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat]), net, opt)
    r = _compare({k: (lambda s=s: s[0](*s[0].static)) for k, s in steps.items()}, 10)
    f, c = r["fused"], r["composition"]
    print("RCAN x4 step, %d groups x %d blocks, 16 x 3 x 48 x 48 -> 192 x 192, replayed graph: fused gate %8.3f ms (rounds "
          "%.3f .. %.3f) | torch composition in its place %8.3f ms (rounds %.3f .. %.3f) = %.2f x"
          % (groups, blocks, f[0], f[1], f[2], c[0], c[1], c[2], c[0] / f[0]), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def parity():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import ca_ref as R
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    worst = {}
    for name in R.cases():
        for skip in (False, True):
            case = R.make(name, skip)
            want = R.restate(case)
            cl = lambda v: v.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            t, x = cl(case.t), (cl(case.x) if skip else None)
            par = [p.to(dev).requires_grad_(True) for p in (case.w1, case.b1, case.w2, case.b2)]
            y = ops.channel_attention(t, x, *par)
            grads = torch.autograd.grad(y, [t] + par, case.g.to(dev).contiguous(memory_format=torch.channels_last))
            errs = {k: R.worst(a, b) for k, a, b in zip(("y", "dt", "dw1", "db1", "dw2", "db2"), (y.detach(),) + grads,
                                                         want[:6]) if float(b.abs().max()) > 0}
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            print("%-12s skip %d  " % (name, skip) + "  ".join("%s %.2e" % kv for kv in errs.items()), flush=True)
    print("worst over the table, of max |ref|:  " + "  ".join("%s %.2e" % kv for kv in worst.items())
          + "   (bars: y 1e-4, gradients 1e-3)", flush=True)


def everything():
    for what, limit in CHILD_LIMITS:
        print("== %s (limit %d s)" % (what, limit), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + what.split(),
                            cwd=ROOT).returncode
        if rc != 0:
            print("== %s ended with status %d: stopping here" % (what, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "all":
        sys.exit(everything())
    if mode == "step":
        step(int(sys.argv[2]), int(sys.argv[3]))
    else:
        {"op": op, "parity": parity}[mode]()
