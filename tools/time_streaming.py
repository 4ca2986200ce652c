#!/usr/bin/env python3
"""Time the streaming entry points at the shapes the nets give them, and the two train steps with the most streaming
launches, with the library SRK_LIB_PATH names (default: this tree's).  Device events around every call; an arm is the
median of 30 warm calls (after 10 of warm-up), a step the median of 30 replays of its hipGraph.
   python tools/time_streaming.py                 one run, one line per arm: "<arm>: <us>"
   python tools/time_streaming.py ab PARENT_LIB [runs]   alternates PARENT_LIB and this tree's library, `runs` (5) fresh
       processes each (the order within a pair swaps every round: the second process of a pair measures slower), and
       prints the table of profiles/streaming_refactor_ab.txt: an arm passes when the tree's median is no slower than the
       slowest of the parent's own runs."""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS, WARM = 30, 10


def median_us(fn):
    import torch
    for _ in range(WARM):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return 1e3 * statistics.median(a.elapsed_time(b) for a, b in ev)


def arms():
    import torch
    import pytorch_super_resolution_model_collection_amd as pkg
    lib, P, S = pkg._lib.load(), pkg._lib.ptr, pkg._lib.stream_ptr
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    r = lambda *s: torch.randn(*s, device=dev)

    def flat(net):      # the length of optim.FlatParams' buffer: every parameter on a 16-byte boundary
        return sum((p.numel() + 3) // 4 * 4 for p in net.parameters())

    n = flat(pkg.EDSRNet(3, 64, 16))
    p, g, m, v = r(n), r(n), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    yield "adam EDSR %d" % n, lambda: lib.srk_adam_step(P(p), P(g), P(m), P(v), n, 1e-4, 0.9, 0.999, 1e-8, 0.0, P(step), None,
                                                       None, S())
    nd = flat(pkg.SRGANDiscriminator(3, 64, 96))
    pd, gd, bd = r(nd), r(nd), torch.zeros(nd, device=dev)
    yield "sgd momentum SRGAN-D %d" % nd, lambda: lib.srk_sgd_step(P(pd), P(gd), P(bd), nd, 1e-4, 0.9, 0.0, 0, 0, None, None, S())
    na = 1 << 20
    dy, y, dx = r(na), r(na), r(na)
    w, dw = torch.full((1,), 0.25, device=dev), torch.zeros(1, device=dev)
    yield "act backward lrelu 1M", lambda: lib.srk_act_backward(P(dy), P(y), P(dx), na, 64, pkg._lib.ACT_LRELU, 0.2, None, 0,
                                                               None, S())
    yield "act backward prelu 1M", lambda: lib.srk_act_backward(P(dy), P(y), P(dx), na, 64, pkg._lib.ACT_PRELU, 0.0, P(w), 1,
                                                               P(dw), S())
    N, C, H, W = 128, 3, 128, 128
    nl = N * C * H * W
    pr, tg, dp, out = torch.rand(nl, device=dev), torch.rand(nl, device=dev), r(nl), torch.zeros(1, device=dev)
    ws = torch.empty(int(lib.srk_loss_workspace_bytes()), dtype=torch.uint8, device=dev)
    nchw = (ctypes.c_int64 * 4)(C * H * W, H * W, W, 1)
    yield "l1 loss 128x3x128x128 dense", lambda: lib.srk_loss_forward_backward(pkg._lib.LOSS_L1, P(pr), P(tg), None, N, C, H, W,
                                                                              0.0, 1.0, P(out), P(dp), P(ws), S())
    yield "l1 loss 128x3x128x128 nchw target", lambda: lib.srk_loss_forward_backward(pkg._lib.LOSS_L1, P(pr), P(tg), nchw, N, C,
                                                                                    H, W, 0.0, 1.0, P(out), P(dp), P(ws), S())
    xm, dym, dxm = r(16 * 128 * 128 * 64), r(16 * 64 * 64 * 64), r(16 * 128 * 128 * 64)
    yield "maxpool backward 16x64x128x128", lambda: lib.srk_maxpool2x2_backward(P(xm), P(dym), P(dxm), 16, 128, 128, 64, 1, S())
    xu, yu = r(16 * 32 * 32 * 64), r(16 * 64 * 64 * 64)
    yield "upsample nearest 16x64x32x32 x2", lambda: lib.srk_upsample_nearest_forward(P(xu), P(yu), 16, 32, 32, 64, 2, S())

    # the steps of bench.py's c4 (EDSR x4, batch 128) and c5 (SRGAN x4, batch 16), built as bench.py builds them
    net = pkg.EDSRNet(3, 64, 16)
    net.weight_init()
    net.to(dev).train()
    fl = pkg.optim.FlatParams(net)
    x, t = torch.rand(128, 3, 32, 32, device=dev), torch.rand(128, 3, 128, 128, device=dev)
    c4 = pkg.trainers.GraphedStep(net, pkg.optim.make_optimizer("edsr", fl, 1e-5), pkg.ops.l1_loss, (x, t), dp=None, clip=None,
                                  warmup=2)
    for sbuf, b in zip(c4.static, (x, t)):
        sbuf.copy_(b)
    yield "c4 EDSR step B=128", lambda: c4(c4.static[0], c4.static[1])
    c4.close()
    G, D = pkg.SRGANGenerator(3, 64, 16), pkg.SRGANDiscriminator(3, 64, 128)
    G.weight_init(), D.weight_init(), G.to(dev).train(), D.to(dev).train()
    gf, df = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    go, do = pkg.optim.make_optimizer("srgan_g", gf, 1e-4), pkg.optim.make_optimizer("srgan_d", df, 1e-4)
    xs, ts = torch.rand(16, 3, 32, 32, device=dev), torch.rand(16, 3, 128, 128, device=dev)
    c5 = pkg.trainers.GraphedFn(pkg.trainers.srgan_step(G, D, go, do, lazy_pack=True), (xs, ts), flats=[gf, df])
    yield "c5 SRGAN step B=16", lambda: c5(xs, ts)


def one_run():
    for name, fn in arms():
        print("%s: %.2f" % (name, median_us(fn)), flush=True)


def ab(parent_lib, runs):
    res = {}
    order = []
    for i in range(runs):
        pair = (("parent", parent_lib), ("tree", None))
        for which, libpath in (pair if i % 2 == 0 else pair[::-1]):      # (neither library always runs behind the other)
            env = dict(os.environ)
            env.pop("SRK_LIB_PATH", None)
            if libpath:
                env["SRK_LIB_PATH"] = os.path.abspath(libpath)
            out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:      # (a fault ends the whole comparison: nothing more is started on the device)
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(out.returncode if out.returncode > 0 else 1)
            for line in out.stdout.splitlines():
                name, us = line.rsplit(": ", 1)
                if name not in order:
                    order.append(name)
                res.setdefault(name, {}).setdefault(which, []).append(float(us))
            print("run %d %s done" % (i + 1, which), file=sys.stderr, flush=True)
    bad = 0
    for name in order:
        pa, tr = res[name]["parent"], res[name]["tree"]
        mp, mt = statistics.median(pa), statistics.median(tr)
        ok = mt <= max(pa)
        bad += not ok
        print(name)
        print("  parent runs %s  median %.2f  min %.2f  max %.2f" % (" ".join("%.2f" % v for v in pa), mp, min(pa), max(pa)))
        print("  tree   runs %s  median %.2f" % (" ".join("%.2f" % v for v in tr), mt))
        print("  tree - parent median %+.2f us (%+.2f %%): %s" % (mt - mp, 100 * (mt - mp) / mp,
                                                                 "inside the parent's spread" if ok else "SLOWER than every parent run"))
    print("\n%s" % ("every arm inside the parent's spread" if not bad else "%d arm(s) slower than every parent run" % bad))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "ab":
        ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        one_run()
