#!/usr/bin/env python3
"""Evidence for DESIGN 27 (LPIPS), run on the MI355X box from the repo root:

  python tools/time_lpips.py op        ops.lpips_layer, forward and forward + backward, against the torch composition of the
                                       same arithmetic (tests/lpips_ref.layer_values: vector_norm, two divisions, sub, mul,
                                       mul, sum, mean) on the same channels_last maps, at the five taps of a [16, 3, 128, 128]
                                       batch and for the five together, each as a fraction of its HBM floor (forward: two
                                       maps read; backward: two read, one written), replayed from captured graphs
  python tools/time_lpips.py term      the whole term ops.lpips at [16, 3, 128, 128], forward and forward + backward,
                                       replayed; and per conv layer of the VGG16 walk the kernel AUTO picks (training
                                       forward) with its time and share
  python tools/time_lpips.py step      one replayed EDSR x4 train step at bench.py's c4 shape (batch 128, 32 x 32 LR) with and
                                       without lpips_weight, and the VGG16 walk's and the distance kernels' parts of it
  python tools/time_lpips.py parity    the layer op and the whole metric against the fp64 restatement on the tests' tables
  python tools/time_lpips.py all       each of the above as a child process under a time limit of its own, stopping at the
                                       first that fails

HIP events; medians over five alternating rounds of `inner` timed calls each, with the lowest and highest round.  The HBM
floor uses 6.3 TB/s, the bandwidth a streaming kernel reaches on this part.  The largest pair of maps is 134 MB and fits the
256 MB last-level cache, so a replayed forward at any tap may be served from it: where a figure is above 100 % of the floor
it is not an HBM figure, and the tool says so."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BATCH = (16, 3, 128, 128)
TAP_SHAPES = ((16, 64, 128, 128), (16, 128, 64, 64), (16, 256, 32, 32), (16, 512, 16, 16), (16, 512, 8, 8))
HBM_BYTES_PER_S = 6.3e12
CHILD_LIMITS = (("parity", 150), ("op", 240), ("term", 240), ("step", 420))


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
    return "%9.2f us (rounds %.2f .. %.2f)" % (1e3 * r[0], 1e3 * r[1], 1e3 * r[2])


def _setup():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    return torch, pkg, torch.device("cuda", 0)


def _floor_note(floor_ms, got_ms):
    pct = 100.0 * floor_ms / got_ms
    return "%.0f %% of the HBM floor %.2f us%s" % (pct, 1e3 * floor_ms, " (above it: served from the last-level cache, not "
                                                  "an HBM figure)" if pct > 100 else "")


def op():
    torch, pkg, dev = _setup()
    import lpips_ref as R
    ops, trainers = pkg.ops, pkg.trainers
    gen = torch.Generator().manual_seed(5)
    maps = []
    for shape in TAP_SHAPES:
        cl = lambda: torch.relu(torch.randn(shape, generator=gen)).to(dev).contiguous(memory_format=torch.channels_last)
        maps.append((cl().requires_grad_(True), cl(), torch.rand(shape[1], generator=gen).to(dev)))
    g64 = torch.full((BATCH[0],), 1.0 / BATCH[0], dtype=torch.float64, device=dev)
    g32 = g64.float()
    table = torch.zeros((5, BATCH[0]), dtype=torch.float64, device=dev)

    def sides_for(idx):
        def fused_fwd():
            with torch.no_grad():
                for l in idx:
                    ops.lpips_layer(maps[l][0], maps[l][1], maps[l][2], l, table)

        def torch_fwd():
            with torch.no_grad():
                for l in idx:
                    R.layer_values(*maps[l])

        def fused():
            for l in idx:
                torch.autograd.grad(ops.lpips_layer(maps[l][0], maps[l][1], maps[l][2], l, table), maps[l][0], g64)

        def composed():
            for l in idx:
                torch.autograd.grad(R.layer_values(*maps[l]), maps[l][0], g32)
        return (("fused fwd", fused_fwd), ("torch fwd", torch_fwd), ("fused", fused), ("torch", composed))

    for name, idx in [("x".join(map(str, s)), (l,)) for l, s in enumerate(TAP_SHAPES)] + [("five taps", tuple(range(5)))]:
        numel = sum(maps[l][0].numel() for l in idx)
        fwd_floor = 2.0 * numel * 4 / HBM_BYTES_PER_S * 1e3
        both_floor = 5.0 * numel * 4 / HBM_BYTES_PER_S * 1e3      # forward: two maps read; backward: two read, one written
        a = torch.autograd.grad(ops.lpips_layer(maps[idx[0]][0], maps[idx[0]][1], maps[idx[0]][2], 0, table), maps[idx[0]][0], g64)[0]
        b = torch.autograd.grad(R.layer_values(*maps[idx[0]]), maps[idx[0]][0], g32)[0]
        diff = float((a - b).abs().max() / b.abs().max())
        graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in sides_for(idx)}
        r = _compare(graphs, 20)
        print("%-16s forward          fused %s | torch composition %s = %.2f x the fused op | %s"
              % (name, _fmt(r["fused fwd"]), _fmt(r["torch fwd"]), r["torch fwd"][0] / r["fused fwd"][0],
                 _floor_note(fwd_floor, r["fused fwd"][0])), flush=True)
        print("%-16s forward+backward fused %s | torch composition %s = %.2f x the fused op | %s | gradients differ by "
              "%.1e of their maximum" % (name, _fmt(r["fused"]), _fmt(r["torch"]), r["torch"][0] / r["fused"][0],
                                         _floor_note(both_floor, r["fused"][0]), diff), flush=True)
        for gr in graphs.values():
            gr.close()


def _net(pkg, dev):
    import lpips_ref as R
    _, _, _, vgg_sd, lin_sd = R.filled_net()
    return pkg.LPIPS(vgg_sd, lin_sd).to(dev).eval()


def term():
    torch, pkg, dev = _setup()
    ops, trainers = pkg.ops, pkg.trainers
    net = _net(pkg, dev)
    gen = torch.Generator().manual_seed(6)
    pred = torch.rand(BATCH, generator=gen).to(dev).requires_grad_(True)
    target = torch.rand(BATCH, generator=gen).to(dev)

    def fwd():
        with torch.no_grad():
            ops.lpips(pred, target, net)

    def both():
        loss = ops.lpips(pred, target, net)
        torch.autograd.grad(loss, pred, ops.unit_seed(dev))
    graphs = {"fwd": trainers.GraphedFn(fwd, (), warmup=2), "both": trainers.GraphedFn(both, (), warmup=2)}
    r = _compare(graphs, 10)
    print("ops.lpips %s replayed: forward (both operands' walks, five distances) %s | forward + backward %s"
          % ("x".join(map(str, BATCH)), _fmt(r["fwd"]), _fmt(r["both"])), flush=True)
    for gr in graphs.values():
        gr.close()
    # the VGG16 walk layer by layer: the kernel the training forward picks, its time, its share
    lib = pkg._lib.load()
    sub, div = ops.lpips_input_affine(True)
    rows, total = [], 0.0
    with torch.no_grad():
        x = ops.channel_affine(target, sub, div)
        for i, m in enumerate(net.features):
            if isinstance(m, torch.nn.Conv2d):
                cfg = ops.ConvCfg(m._s, m._p, False, 0, pkg._lib.ACT_RELU)
                packed = m._cache.get(m.weight, m.bias, False, 0, bwd=True)
                call = lambda x=x, m=m, cfg=cfg, packed=packed: ops.conv2d(x, m.weight, m.bias, None, cfg, packed)
                y = call()
                name = lib.srk_last_kernel_name().decode()
                ms = statistics.median(_events(call, 10) for _ in range(3))
                rows.append((i, tuple(x.shape), m.out_channels, name, ms))
                total += ms
                x = y
            elif not isinstance(m, torch.nn.ReLU):
                x = ops.max_pool2x2(x)
    for i, shape, cout, name, ms in rows:
        flops = 2.0 * shape[0] * shape[2] * shape[3] * shape[1] * cout * 9
        print("features.%-2d conv %3d -> %3d on %3d x %3d  %-34s %8.2f us  %5.1f %% of the walk's convs  %6.1f TFLOP/s"
              % (i, shape[1], cout, shape[2], shape[3], name, 1e3 * ms, 100 * ms / total, flops / ms / 1e9), flush=True)
    print("one operand's 13 convs, training forward, called one by one: %.2f us" % (1e3 * total), flush=True)


def step():
    torch, pkg, dev = _setup()
    from oracle import fill
    net = _net(pkg, dev)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((128, 3, 32, 32), generator=gen).to(dev), torch.rand((128, 3, 128, 128), generator=gen).to(dev)
    steps = {}
    for side, kw in (("plain", {}), ("lpips", {"lpips_weight": 0.1, "lpips_net": net})):
        model = pkg.EDSRNet(3, 64, 16)
        fill.fill_module(model, 3, 0.5)
        model.to(dev).train()
        flat, opt, dp, eager = pkg.trainers.build("edsr", model, 1e-5, **kw)
        steps[side] = (pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat]), model, opt)
    r = _compare({k: (lambda s=s: s[0](*s[0].static)) for k, s in steps.items()}, 5)
    p, l = r["plain"], r["lpips"]
    print("EDSR x4 step, 128 x 3 x 32 x 32 -> 128 x 128, replayed graph: L1 alone %8.3f ms (rounds %.3f .. %.3f) | with "
          "lpips_weight 0.1 %8.3f ms (rounds %.3f .. %.3f) = %.2f x" % (p[0], p[1], p[2], l[0], l[1], l[2], l[0] / p[0]),
          flush=True)
    for s in steps.values():
        s[0].close()
    # the term alone on the step's HR batch, and its five distances alone on maps of the step's sizes
    ops = pkg.ops
    pred = tgt.clone().mul_(0.9).requires_grad_(True)

    def whole():
        torch.autograd.grad(ops.lpips(pred, tgt, net), pred, ops.unit_seed(dev))
    with torch.no_grad():
        sub, div = ops.lpips_input_affine(True)
        fa = net.extract(ops.channel_affine(pred.detach(), sub, div), grad=True)
        fb = net.extract(ops.channel_affine(tgt, sub, div), grad=True)
    fa = [f.detach().requires_grad_(True) for f in fa]
    table = torch.zeros((5, 128), dtype=torch.float64, device=dev)
    g64 = torch.full((128,), 1.0 / 128, dtype=torch.float64, device=dev)

    def distances():
        for i, (a, b, w) in enumerate(zip(fa, fb, net.lins)):
            torch.autograd.grad(ops.lpips_layer(a, b, w, i, table), a, g64)
    graphs = {"term": pkg.trainers.GraphedFn(whole, (), warmup=1), "distances": pkg.trainers.GraphedFn(distances, (), warmup=1)}
    r = _compare(graphs, 5)
    print("of that, measured alone at the step's HR batch: the whole term forward + backward %8.3f ms (rounds %.3f .. %.3f); "
          "its five distance layers forward + backward %8.3f ms (rounds %.3f .. %.3f) = %.1f %% of the term; the rest is "
          "the two VGG16 walks and the one backward through them"
          % (r["term"] + r["distances"] + (100 * r["distances"][0] / r["term"][0],)), flush=True)
    for gr in graphs.values():
        gr.close()


def parity():
    torch, pkg, dev = _setup()
    import lpips_ref as R
    ops = pkg.ops
    for shape in R.LAYER_SHAPES:
        case = R.layer_case(shape)
        a = case["f0"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        b = case["f1"].to(dev).contiguous(memory_format=torch.channels_last)
        table = torch.zeros((1, shape[0]), dtype=torch.float64, device=dev)
        v = ops.lpips_layer(a, b, case["w"].to(dev), 0, table)
        v.backward(case["g"].to(dev))
        ve, vs = R.max_err(v, case["value"])
        ge, gs = R.max_err(a.grad, case["df0"])
        print("layer %-16s value err %.3g of max |ref| %.3g (bar %.3g)  gradient err %.3g of %.3g (bar %.3g)"
              % (shape, ve, vs, R.OUT_CONTRACT * vs, ge, gs, R.GRAD_CONTRACT * gs), flush=True)
    net = _net(pkg, dev)
    for shape in R.METRIC_SHAPES:
        for normalize in (True, False):
            case = R.metric_case(shape, normalize)
            pred = case["pred"].to(dev).requires_grad_(True)
            target = case["target"].to(dev)
            values = ops.lpips(pred.detach(), target, net, normalize, reduce=False)
            ops.backward(ops.lpips(pred, target, net, normalize))
            ve, vs = R.max_err(values, case["v64"])
            ge, gs = R.max_err(pred.grad, case["d64"])
            print("metric %-16s normalize %d  value err %.3g (torch fp32 CPU %.3g; contract %.3g; bar %.3g)  gradient err %.3g "
                  "(torch fp32 CPU %.3g; contract %.3g; bar %.3g)"
                  % (shape, normalize, ve, case["v_err32"], R.OUT_CONTRACT * vs, R.bar(R.OUT_CONTRACT, case["v_err32"], vs),
                     ge, case["d_err32"], R.GRAD_CONTRACT * gs, R.bar(R.GRAD_CONTRACT, case["d_err32"], gs)), flush=True)


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
    {"op": op, "term": term, "step": step, "parity": parity}[mode]()
