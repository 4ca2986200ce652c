#!/usr/bin/env python3
"""Evidence for DESIGN 28 (slice convolutions, RDN), run on the MI355X box from the repo root:

  python tools/time_rdn.py block        one residual dense block, forward and forward + backward, at [16, 64, 32, 32] and
                                        [16, 64, 48, 48] with (C, G) = (8, 64) and (6, 32): ops.residual_dense_blocks against
                                        the composition it replaces -- torch.cat + ops.conv2d on the existing kernels, same
                                        precision mode, filters packed once outside the timed region (what optim.PackPlan
                                        gives a net) -- replayed from captured graphs; with the fused path's TFLOP/s against
                                        the 3-MFMA peak and its bytes against the algorithmic minimum
  python tools/time_rdn.py step 2 3 32  one replayed RDN x4 train step (batch 16, 32 x 32 LR, Adam, L1) of D = 2 blocks of
  python tools/time_rdn.py step 16 8 64 C = 3 layers with G = 32 / of the paper's net, against the same net built on
                                        layers.Conv2d and torch.cat (its filters in the PackPlan)
  python tools/time_rdn.py parity       the raw operator and the trunk against the fp64 restatement on the tests' case
                                        table: worst error per output over max |ref| (bars 1e-4 forward, 1e-3 gradients)
  python tools/time_rdn.py all          each of the above as a child process under a time limit of its own, stopping at the
                                        first that fails

HIP events; medians over five alternating rounds of 20 timed replays (steps: 5) each, with the min and max of the round
medians.  FLOPs: 2 * N H W * sum over the block's layers of K^2 Cin Cout, three times that for forward + backward; the
peak is 2.5 PF / 3 MFMAs per product (the backward's arithmetic; the mixed mode's training forward runs six).  Bytes: the
algorithmic minimum reads the block input and writes every layer output once (forward), and for the backward reads the
output gradient, the input and every layer output once and writes the input gradient once; weights are left out."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((16, 64, 32, 32), (16, 64, 48, 48))
CONFIGS = ((8, 64), (6, 32))
MFMA3_PEAK = 2500e12 / 3.0
HBM_BYTES_PER_S = 6.3e12
CHILD_LIMITS = (("parity", 150), ("block", 240), ("step 2 3 32", 150), ("step 16 8 64", 400))


def _events(fn, inner, warm=2):
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
    return "%9.1f us (rounds %.1f .. %.1f)" % (1e3 * r[0], 1e3 * r[1], 1e3 * r[2])


def _composed_block(ops, x, params, packed, fork, keep=None):
    """The block as today's ops express it: a cat in front of every layer.  keep: a list that receives the layer outputs."""
    import torch
    from pytorch_super_resolution_model_collection_amd._lib import ACT_RELU
    C = len(params) // 2 - 1
    feats = x
    for c in range(C):
        y = ops.conv2d(feats, params[2 * c], params[2 * c + 1], None, ops.ConvCfg(1, 1, False, 0, ACT_RELU, 0.0, 0),
                       packed[c] if fork else None) if fork else \
            ops.conv2d_infer(feats, params[2 * c], params[2 * c + 1], None, ops.ConvCfg(1, 1, False, 0, ACT_RELU, 0.0, 0),
                             None, packed[c][:2])
        if keep is not None:
            keep.append(y.detach())
        feats = torch.cat((feats, y), 1)
    if fork:
        return ops.conv2d(feats, params[2 * C], params[2 * C + 1], x, ops.ConvCfg(1, 0), packed[C])
    return ops.conv2d_infer(feats, params[2 * C], params[2 * C + 1], x, ops.ConvCfg(1, 0), None, packed[C][:2])


def block():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import rdn_ref as R
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    print("precision mode %s: training forward on %d MFMAs a product, backward on %d, inference on %d"
          % (ops.get_precision(), ops.dense_terms("train_fwd"), ops.dense_terms("bwd"), ops.dense_terms("infer")), flush=True)
    for shape in SHAPES:
        for C, G in CONFIGS:
            n, g0, h, w = shape
            params = [p.to(dev).requires_grad_(True) for p in R.make_blocks(g0, G, C, 1, 11)[0]]
            x = R.rand(shape, 5).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = R.rand(shape, 6).to(dev).contiguous(memory_format=torch.channels_last)
            packed = [(ops.pack_weight_fwd(params[2 * c].detach(), False, 0), params[2 * c + 1],
                       ops.pack_weight_bwd(params[2 * c].detach(), False, 0)) for c in range(C + 1)]
            leaves = [x] + params

            def fused_fwd():
                with torch.no_grad():
                    ops.residual_dense_blocks(x, [params])

            def cat_fwd():
                with torch.no_grad():
                    _composed_block(ops, x, params, packed, False)

            def fused():
                torch.autograd.grad(ops.residual_dense_blocks(x, [params]), leaves, g)

            def composed():
                torch.autograd.grad(_composed_block(ops, x, params, packed, True), leaves, g)

            out_a, ys = ops.residual_dense_blocks(x, [params]), []
            growth = out_a.grad_fn.saved_tensors[2]          # the slice path's layer outputs = its ReLU masks
            a = torch.autograd.grad(out_a, leaves, g)
            del out_a    # no autograd graph may outlive this comparison: a node kept from here (and the AccumulateGrad
            #              nodes of the leaves with it) would be synchronised with inside the stream captures below
            b = torch.autograd.grad(_composed_block(ops, x, params, packed, True, ys), leaves, g)
            per = [float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b)]
            diff = max(per)
            # where the two gradients part: the two forwards round differently, so a layer output within rounding of zero
            # is positive in one and zero in the other, and that unit's whole contribution to dx is present in one
            # backward and absent in the other
            comp = torch.cat(ys, 1)
            flipped = int(((growth > 0) != (comp > 0)).sum())
            fwd_diff = float((growth - comp).abs().max() / comp.abs().max())
            dx_far = int(((a[0] - b[0]).abs() > 1e-3 * b[0].abs().max()).sum())
            names = ["dx"] + ["%s%d" % ("w" if i % 2 == 0 else "b", i // 2 + 1) for i in range(len(params))]
            print("%s C=%d G=%d  the two paths compared: layer outputs differ by %.1e of their maximum; %d of %d ReLU "
                  "masks differ; gradients apart by  " % ("x".join(map(str, shape)), C, G, fwd_diff, flipped, growth.numel())
                  + "  ".join("%s %.1e" % nv for nv in zip(names, per))
                  + "   (%d of %d dx elements further apart than 1e-3 of the maximum)" % (dx_far, a[0].numel()), flush=True)
            del growth, comp, ys
            graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in
                      (("fused fwd", fused_fwd), ("cat fwd", cat_fwd), ("fused", fused), ("cat", composed))}
            r = _compare(graphs, 20)
            P = n * h * w
            flop = 2.0 * P * (sum(9 * (g0 + c * G) * G for c in range(C)) + (g0 + C * G) * g0)
            fwd_bytes = 4.0 * P * (g0 + C * G + g0)
            bwd_bytes = 4.0 * P * (g0 + g0 + C * G + g0)
            tag = "%s C=%d G=%d" % ("x".join(map(str, shape)), C, G)
            print("%-26s forward          slices %s | cat + conv2d %s = %.2f x the slice path | %.1f TFLOP/s = %.1f %% of the "
                  "3-MFMA peak | %.1f MB minimum = %.1f us at 6.3 TB/s"
                  % (tag, _fmt(r["fused fwd"]), _fmt(r["cat fwd"]), r["cat fwd"][0] / r["fused fwd"][0],
                     flop / (r["fused fwd"][0] * 1e-3) / 1e12, 100 * flop / (r["fused fwd"][0] * 1e-3) / MFMA3_PEAK,
                     fwd_bytes / 1e6, fwd_bytes / HBM_BYTES_PER_S * 1e6), flush=True)
            print("%-26s forward+backward slices %s | cat + conv2d %s = %.2f x the slice path | %.1f TFLOP/s = %.1f %% of the "
                  "3-MFMA peak | %.1f MB minimum = %.1f us | gradients of the two differ by %.1e of their maximum"
                  % (tag, _fmt(r["fused"]), _fmt(r["cat"]), r["cat"][0] / r["fused"][0],
                     3 * flop / (r["fused"][0] * 1e-3) / 1e12, 300 * flop / (r["fused"][0] * 1e-3) / MFMA3_PEAK,
                     (fwd_bytes + bwd_bytes) / 1e6, (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S * 1e6, diff), flush=True)
            for gr in graphs.values():
                gr.close()


def _composed_net(pkg, D, C, G):
    """RDNNet's twin on layers.Conv2d and torch.cat: the same parameters under the same names, every filter in the
    PackPlan, a cat in front of every layer of every block and one in front of GFF."""
    import torch
    from pytorch_super_resolution_model_collection_amd import layers, ops
    from pytorch_super_resolution_model_collection_amd._lib import ACT_RELU

    class Layer(torch.nn.Module):
        def __init__(self, cin, g):
            super().__init__()
            self.conv = torch.nn.Sequential(layers.Conv2d(cin, g, 3, 1, 1), layers.ReLU())

    class Block(torch.nn.Module):
        def __init__(self, g0, g, c):
            super().__init__()
            self.convs = torch.nn.Sequential(*[Layer(g0 + i * g, g) for i in range(c)])
            self.LFF = layers.Conv2d(g0 + c * g, g0, 1, 1, 0)

        def forward(self, x):
            feats = x
            for m in self.convs:
                feats = torch.cat((feats, m.conv[0].run(feats, ACT_RELU)), 1)
            return self.LFF.run(feats, residual=x)

    class Net(pkg.RDNNet):
        def __init__(self):
            super().__init__(3, 64, D, C, G, 4)
            self.RDBs = torch.nn.ModuleList([Block(64, G, C) for _ in range(D)])

        def forward(self, x):
            f1 = self.SFENet1(x)
            h, outs = self.SFENet2(f1), []
            for b in self.RDBs:
                h = b(h)
                outs.append(h)
            out = self.GFF[1].run(self.GFF[0](torch.cat(outs, 1)), residual=f1)
            for m in self.UPNet:
                if isinstance(m, layers.Conv2d):
                    out = m.run(out, ps_r=getattr(m, "_ps_r", 0))
            return out
    return Net()


def step(D, C, G):
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((16, 3, 32, 32), generator=gen).to(dev), torch.rand((16, 3, 128, 128), generator=gen).to(dev)
    steps = {}
    for side in ("slices", "cat"):
        net = pkg.RDNNet(3, 64, D, C, G, 4) if side == "slices" else _composed_net(pkg, D, C, G)
        fill.fill_module(net, 3, 0.3)
        net.to(dev).train()
        flat, opt, dp, eager = pkg.trainers.build("rdn", net, 1e-5)
        steps[side] = (pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat]), net, opt)
    r = _compare({k: (lambda s=s: s[0](*s[0].static)) for k, s in steps.items()}, 5)
    f, c = r["slices"], r["cat"]
    print("RDN x4 step, D = %d, C = %d, G = %d, 16 x 3 x 32 x 32 -> 128 x 128, replayed graph: slice convolutions %9.3f ms "
          "(rounds %.3f .. %.3f) | torch.cat + layers.Conv2d in their place %9.3f ms (rounds %.3f .. %.3f) = %.2f x"
          % (D, C, G, f[0], f[1], f[2], c[0], c[1], c[2], c[0] / f[0]), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def parity():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import rdn_ref as R
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    worst = {}
    for name in sorted(R.CASES):
        c = R.case(name)
        a, b = c.A.device(dev), (c.B.device(dev) if c.B else None)
        wt, bias, dy, ys = c.W.to(dev), c.bias.to(dev), c.DY.device(dev), c.YS.device(dev)
        act = c.act != R.ACT_NONE
        y = ops.dense_conv(a, wt, bias, b, None, c.ca, c.A.off, c.cb, c.B.off if c.B else 0, 0, c.act, R.SLOPE,
                           c.R.device(dev) if c.R else None, c.R.off if c.R else 0, c.terms)
        n, h, w = c.dims
        da = torch.empty((n, c.ca, h, w), device=dev).contiguous(memory_format=torch.channels_last)
        db = torch.empty((n, c.cb, h, w), device=dev).contiguous(memory_format=torch.channels_last) if c.cb else None
        ops.dense_conv_backward_data(dy, wt, c.ca, c.cb, ys if act else None, da, db, None, c.DY.off, c.YS.off, 0, 0, 0, 0.0,
                                     0.0, c.act, R.SLOPE, c.terms)
        dw, dbias = torch.empty_like(wt), torch.empty_like(bias)
        ops.dense_conv_backward_weight(a, dy, dw, dbias, b, ys if act else None, c.ca, c.A.off, c.cb, c.B.off if c.B else 0,
                                       c.DY.off, c.YS.off, 0.0, c.act, R.SLOPE, c.terms)
        errs = {"y": R.worst(y, c.y), "dA": R.worst(da, c.da), "dW": R.worst(dw, c.dw), "db": R.worst(dbias, c.dbias)}
        if db is not None:
            errs["dB"] = R.worst(db, c.db)
        for k, v in errs.items():
            worst[(c.terms, k)] = max(worst.get((c.terms, k), 0.0), v)
        print("%-20s terms %d  " % (name, c.terms) + "  ".join("%s %.2e" % kv for kv in sorted(errs.items())), flush=True)
    for terms in (3, 6):
        print("worst over the table at %d terms, of max |ref|:  " % terms
              + "  ".join("%s %.2e" % (k[1], v) for k, v in sorted(worst.items()) if k[0] == terms)
              + "   (bars: y 1e-4, gradients 1e-3)", flush=True)
    for g0, g, C, D in ((16, 16, 3, 2), (64, 32, 2, 2)):
        blocks = R.make_blocks(g0, g, C, D, 40 + g0)
        x, gy = R.rand((2, g0, 12, 10), 3), R.rand((2, D * g0, 12, 10), 4)
        x64 = x.double().requires_grad_(True)
        b64 = [tuple(p.double().requires_grad_(True) for p in b) for b in blocks]
        R.trunk_forward(x64, b64).backward(gy.double())
        want = R.trunk_forward(x64, b64).detach()
        xd = x.to(dev).requires_grad_(True)
        bd = [tuple(p.to(dev).requires_grad_(True) for p in b) for b in blocks]
        got = ops.residual_dense_blocks(xd, bd)
        got.backward(gy.to(dev))
        eg = max(R.worst(p.grad, q.grad) for b, c in zip(bd, b64) for p, q in zip(b, c))
        print("trunk G0 %d G %d C %d D %d (mode %s): output %.2e  dx %.2e  worst parameter gradient %.2e of max |ref|"
              % (g0, g, C, D, ops.get_precision(), R.worst(got.detach(), want), R.worst(xd.grad, x64.grad), eg), flush=True)


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
        step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        {"block": block, "parity": parity}[mode]()
