#!/usr/bin/env python3
"""Evidence for DESIGN 29 (shifted-window attention, LayerNorm, GELU, SwinIR), run on the MI355X box from the repo root:

  python tools/time_wattn.py op         ops.window_attention, forward and forward + backward, against the torch composition
                                        it replaces (roll, partition, bmm, bias gather, mask add, softmax, bmm, reverse,
                                        roll: tests/swinir_ref.py in fp32 with the index and mask tensors built once) at
                                        [16, 48, 48, 180] and [16, 64, 64, 60] (6 heads, window 8, shift 4) and the same at
                                        N = 1, with the fraction of the two floors each reaches
  python tools/time_wattn.py pointwise  ops.layer_norm and ops.gelu against ATen at [36864, 180]
  python tools/time_wattn.py convs      which existing conv kernel the 60- and 180-channel 1x1 and 3x3 layers of the net
                                        dispatch to, and at what TFLOP/s
  python tools/time_wattn.py step light / step dim180
                                        one replayed SwinIR x4 train step (batch 16, 48 x 48 LR, Adam, L1) of the
                                        lightweight net / of a 2 x 2-layer net at dim 180, with the three operators and
                                        with their torch compositions in their place
  python tools/time_wattn.py parity     the op against the fp64 restatement on the case table of the tests
  python tools/time_wattn.py all        each of the above as a child process under a time limit of its own, stopping at
                                        the first that fails

Everything is a replayed graph; HIP events; medians over five alternating rounds of 20 timed replays (steps: 5) each,
with the min and max of the round medians.  Floors at a shape: the kernel must read qkv and write the result (forward:
16 N H W C bytes) and read qkv, the result, its gradient and write dqkv (backward: 32 N H W C bytes), over 8 TB/s;
Q K^T and P V are 2 * 2 * T * d FLOP per token and head, the backward five such products, over the 157 TFLOP/s fp32
vector rate."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((16, 48, 48, 180), (16, 64, 64, 60), (1, 48, 48, 180), (1, 64, 64, 60))
HEADS, WINDOW, SHIFT = 6, 8, 4
HBM_BYTES_PER_S, FP32_FLOPS = 8.0e12, 157e12
CHILD_LIMITS = (("parity", 120), ("op", 240), ("pointwise", 120), ("convs", 180), ("step light", 400), ("step dim180", 300))


def _events(fn, inner, warm=2):
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
    res = {k: [] for k in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            res[name].append(_events(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def _fmt(r):
    return "%8.2f us (rounds %.2f .. %.2f)" % (1e3 * r[0], 1e3 * r[1], 1e3 * r[2])


class Composition(object):
    """The torch composition of the operator in fp32, index and mask tensors built once (as upstream's buffers are)."""

    def __init__(self, h, w, heads, window, shift, dev):
        import swinir_ref as R
        self.R, self.heads, self.window, self.shift = R, heads, window, shift
        self.index = R.rel_index(window).flatten().to(dev)
        self.mask = R.mask_tensor(h, w, window, shift).float().to(dev) if shift else None

    def __call__(self, qkv, table):
        import torch
        R, heads, window, shift = self.R, self.heads, self.window, self.shift
        n, h, w, c3 = qkv.shape
        c = c3 // 3
        d = c // heads
        x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
        wins = R.partition(x, window)
        b, t, _ = wins.shape
        q, k, v = wins.view(b, t, 3, heads, d).permute(2, 0, 3, 1, 4)
        s = (q * d ** -0.5) @ k.transpose(-2, -1)
        s = s + table[self.index].view(t, t, heads).permute(2, 0, 1)[None]
        if self.mask is not None:
            s = (s.view(n, -1, heads, t, t) + self.mask[None, :, None]).view(b, heads, t, t)
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, t, c)
        o = R.reverse(o, window, n, h, w)
        return torch.roll(o, (shift, shift), (1, 2)) if shift else o


def op():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    for shape in SHAPES:
        n, h, w, c = shape
        qkv = torch.randn((n, h, w, 3 * c), generator=gen).to(dev).requires_grad_(True)
        table = torch.randn(((2 * WINDOW - 1) ** 2, HEADS), generator=gen).to(dev).requires_grad_(True)
        g = torch.randn(shape, generator=gen).to(dev)
        comp = Composition(h, w, HEADS, WINDOW, SHIFT, dev)
        leaves = [qkv, table]

        def fused_fwd():
            with torch.no_grad():
                ops.window_attention(qkv, table, HEADS, WINDOW, SHIFT)

        def torch_fwd():
            with torch.no_grad():
                comp(qkv, table)

        def fused():
            torch.autograd.grad(ops.window_attention(qkv, table, HEADS, WINDOW, SHIFT), leaves, g)

        def composed():
            torch.autograd.grad(comp(qkv, table), leaves, g)

        a = torch.autograd.grad(ops.window_attention(qkv, table, HEADS, WINDOW, SHIFT), leaves, g)
        b = torch.autograd.grad(comp(qkv, table), leaves, g)
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in
                  (("fused fwd", fused_fwd), ("torch fwd", torch_fwd), ("fused", fused), ("torch", composed))}
        r = _compare(graphs, 20)
        tokens, d = n * h * w, c // HEADS
        mem_f, mem_b = 16.0 * tokens * c / HBM_BYTES_PER_S * 1e3, 32.0 * tokens * c / HBM_BYTES_PER_S * 1e3      # ms
        fma_f = 4.0 * WINDOW * WINDOW * d * tokens * HEADS / FP32_FLOPS * 1e3
        fma_b = 2.5 * fma_f
        name = "x".join(map(str, shape))
        print("%-14s forward          fused %s | torch composition %s = %.2f x the fused op | floors: HBM %.1f us (%.0f %% "
              "reached), FMA %.1f us (%.0f %%)" % (name, _fmt(r["fused fwd"]), _fmt(r["torch fwd"]),
                                                   r["torch fwd"][0] / r["fused fwd"][0], 1e3 * mem_f,
                                                   100 * mem_f / r["fused fwd"][0], 1e3 * fma_f,
                                                   100 * fma_f / r["fused fwd"][0]), flush=True)
        fb, tb = r["fused"][0], r["torch"][0]
        print("%-14s forward+backward fused %s | torch composition %s = %.2f x the fused op | floors: HBM %.1f us (%.0f %% "
              "reached), FMA %.1f us (%.0f %%) | gradients of the two differ by %.1e of their maximum"
              % (name, _fmt(r["fused"]), _fmt(r["torch"]), tb / fb, 1e3 * (mem_f + mem_b), 100 * (mem_f + mem_b) / fb,
                 1e3 * (fma_f + fma_b), 100 * (fma_f + fma_b) / fb, diff), flush=True)
        for gr in graphs.values():
            gr.close()


def pointwise():
    import torch
    import torch.nn.functional as F
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(6)
    rows, c = 36864, 180
    x = torch.randn((rows, c), generator=gen).to(dev).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(c, generator=gen)).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(c, generator=gen)).to(dev).requires_grad_(True)
    g = torch.randn((rows, c), generator=gen).to(dev)
    sides = {
        "layer_norm fused": lambda: torch.autograd.grad(ops.layer_norm(x, gamma, beta), [x, gamma, beta], g),
        "layer_norm ATen": lambda: torch.autograd.grad(F.layer_norm(x, (c,), gamma, beta), [x, gamma, beta], g),
        "gelu fused": lambda: torch.autograd.grad(ops.gelu(x), [x], g),
        "gelu ATen": lambda: torch.autograd.grad(F.gelu(x), [x], g),
    }

    def nograd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run
    sides.update({"layer_norm fused fwd": nograd(lambda: ops.layer_norm(x, gamma, beta)),
                  "layer_norm ATen fwd": nograd(lambda: F.layer_norm(x, (c,), gamma, beta)),
                  "gelu fused fwd": nograd(lambda: ops.gelu(x)), "gelu ATen fwd": nograd(lambda: F.gelu(x))})
    graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in sides.items()}
    r = _compare(graphs, 20)
    one_pass = rows * c * 4 / HBM_BYTES_PER_S * 1e3
    for what, passes_f, passes_fb in (("layer_norm", 2, 5), ("gelu", 2, 5)):
        print("%-10s [%d, %d] forward          fused %s | ATen %s | HBM floor %.1f us" % (
            what, rows, c, _fmt(r[what + " fused fwd"]), _fmt(r[what + " ATen fwd"]), 1e3 * passes_f * one_pass), flush=True)
        print("%-10s [%d, %d] forward+backward fused %s | ATen %s | HBM floor %.1f us" % (
            what, rows, c, _fmt(r[what + " fused"]), _fmt(r[what + " ATen"]), 1e3 * passes_fb * one_pass), flush=True)
    for gr in graphs.values():
        gr.close()


def convs():
    """The net's conv layers at the trainer's [16, C, 48, 48]: the kernel each direction dispatches to, and its rate."""
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd import layers, ops
    lib = pkg._lib.load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(7)
    for cin, cout, k in ((60, 180, 1), (60, 60, 1), (60, 120, 1), (120, 60, 1), (60, 60, 3),
                         (180, 540, 1), (180, 180, 1), (180, 360, 1), (360, 180, 1), (180, 180, 3)):
        m = (layers.TokenLinear(cin, cout) if k == 1 else layers.Conv2d(cin, cout, 3, 1, 1)).to(dev)
        x = torch.randn((16, cin, 48, 48), generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        y = m.run(x)
        fwd_name = lib.srk_last_kernel_name().decode()
        g = torch.randn(y.shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        y.backward(g)
        ops.flush_wgrads()
        bwd_name = lib.srk_last_kernel_name().decode()

        def fwd():
            m.run(x)

        def both():
            m.run(x).backward(g)
            ops.flush_wgrads()
        r = _compare({"fwd": fwd, "both": both}, 10, rounds=3)
        flop = 2.0 * 16 * 48 * 48 * cin * cout * k * k
        generic = "generic" in fwd_name.lower() or "generic" in bwd_name.lower()
        print("%dx%d %3d -> %3d  forward %s %6.1f TFLOP/s [%s] | forward + both gradients %s %6.1f TFLOP/s [last: %s]%s"
              % (k, k, cin, cout, _fmt(r["fwd"]), flop / r["fwd"][0] / 1e9, fwd_name, _fmt(r["both"]),
                 3 * flop / r["both"][0] / 1e9, bwd_name, "  ** GENERIC KERNEL **" if generic else ""), flush=True)


class _Composed(object):
    """The three operators replaced by their torch compositions inside the package's modules (the timing's other side)."""

    def __enter__(self):
        import torch.nn.functional as F
        from pytorch_super_resolution_model_collection_amd import ops
        self.ops, self.old = ops, (ops.window_attention, ops.layer_norm, ops.gelu)
        comps = {}

        def wattn(qkv, table, heads, window, shift=0):
            key = (qkv.shape[1], qkv.shape[2], heads, window, shift)
            if key not in comps:
                comps[key] = Composition(qkv.shape[1], qkv.shape[2], heads, window, shift, qkv.device)
            return comps[key](qkv, table)
        ops.window_attention = wattn
        ops.layer_norm = lambda x, gamma, beta, eps=1e-5: F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
        ops.gelu = lambda x: F.gelu(x)
        return self

    def __exit__(self, *a):
        self.ops.window_attention, self.ops.layer_norm, self.ops.gelu = self.old


def step(which):
    import contextlib
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    ctor = {"light": (3, 60, (6, 6, 6, 6), 6, 8, 2, 4, "pixelshuffledirect"),
            "dim180": (3, 180, (2, 2), 6, 8, 2, 4, "pixelshuffle")}[which]
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((16, 3, 48, 48), generator=gen).to(dev), torch.rand((16, 3, 192, 192), generator=gen).to(dev)
    steps = {}
    for side in ("fused", "composition"):
        ctx = _Composed() if side == "composition" else contextlib.nullcontext()
        with ctx:
            net = pkg.SwinIRNet(*ctor)
            fill.fill_module(net, 3, 0.1)
            net.to(dev).train()
            flat, opt, dp, eager = pkg.trainers.build("swinir", net, 1e-5)
            steps[side] = (pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat]), net, opt, ctx)
    r = _compare({k: (lambda s=s: s[0](*s[0].static)) for k, s in steps.items()}, 5)
    f, c = r["fused"], r["composition"]
    print("SwinIR x4 step %s %s, 16 x 3 x 48 x 48 -> 192 x 192, replayed graph: fused operators %8.3f ms (rounds %.3f .. "
          "%.3f) | torch compositions in their place %8.3f ms (rounds %.3f .. %.3f) = %.2f x"
          % (which, ctor, f[0], f[1], f[2], c[0], c[1], c[2], c[0] / f[0]), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def parity():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import swinir_ref as R
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    worst = {}
    for name, case in R.CASES.items():
        n, h, w, c, heads, window, shift = case
        want = R.attention_with_grads(case)
        qkv, table, g = R.inputs(case)
        qkv, table = qkv.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
        out = ops.window_attention(qkv, table, heads, window, shift)
        grads = torch.autograd.grad(out, [qkv, table], g.to(dev))
        errs = {k: R.worst(a, b) for k, a, b in zip(("out", "dqkv", "dtable"), (out.detach(),) + grads, want)}
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print("%-16s %s  " % (name, case) + "  ".join("%s %.2e" % kv for kv in errs.items()), flush=True)
    print("worst over the table, of max |ref|:  " + "  ".join("%s %.2e" % kv for kv in worst.items())
          + "   (bars: out 1e-4, gradients 1e-3)", flush=True)


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
        step(sys.argv[2])
    else:
        {"op": op, "pointwise": pointwise, "convs": convs, "parity": parity}[mode]()
