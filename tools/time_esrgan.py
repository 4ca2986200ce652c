#!/usr/bin/env python3
"""Evidence for DESIGN 30 (ESRGAN), run on the MI355X box from the repo root:

  python tools/time_esrgan.py block      one RRDB (F = 64, G = 32) at [16, 64, 32, 32], forward and forward + backward:
                                         ops.rrdb_trunk against the composition it replaces -- torch.cat + ops.conv2d (the
                                         LeakyReLU fused into the conv, filters packed once outside the timed region) + srk_axpby
                                         for every scaled skip -- in the same precision mode, replayed from captured graphs
  python tools/time_esrgan.py ragan      ops.ragan_loss forward + backward at B = 16 against the torch composition
  python tools/time_esrgan.py step NB    one replayed ESRGAN adversarial step (batch 16, 32 x 32 LR, 128 x 128 HR) with NB
                                         blocks; the VGG head carries seeded random weights (the time does not depend on them)
  python tools/time_esrgan.py parity     the new GPU tests with their printed errors (worst error over max |fp64 ref|)
  python tools/time_esrgan.py all        each of the above as a child process under a time limit of its own, stopping at
                                         the first that fails

HIP events; medians over five alternating rounds of 20 timed replays (steps: 5) each, with the min and max of the round
medians."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHILD_LIMITS = (("parity", 300), ("block", 200), ("ragan", 100), ("step 2", 200), ("step 23", 400))
RS = 0.2


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
    """{name: fn} -> {name: (median, min, max of the round medians) ms per call}, the sides alternated"""
    res = {k: [] for k in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            res[name].append(_events(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def _fmt(r):
    return "%9.1f us (rounds %.1f .. %.1f)" % (1e3 * r[0], 1e3 * r[1], 1e3 * r[2])


def _axpby_fn(ops):
    import torch

    class Axpby(torch.autograd.Function):
        """alpha * a + b on srk_axpby, differentiable in both (the composition's scaled skip)."""

        @staticmethod
        def forward(ctx, a, b, alpha):
            ctx.alpha = alpha
            return ops._axpby(a, b, alpha, 1.0)

        @staticmethod
        def backward(ctx, g):
            return ops._axpby(g, g, ctx.alpha, 0.0), g, None
    return Axpby.apply


def _composed_rrdb(ops, x, rrdb, packed, grad, axpby):
    """The RRDB as the ops before this section express it: a cat in front of every conv, a launch for every scaled skip."""
    import torch
    from pytorch_super_resolution_model_collection_amd._lib import ACT_LRELU, ACT_NONE
    u = x
    for k, p in enumerate(rrdb):
        feats = u
        for c in range(5):
            cfg = ops.ConvCfg(1, 1, False, 0, ACT_LRELU if c < 4 else ACT_NONE, 0.2, 0)
            pk = packed[k][c]
            y = ops.conv2d(feats, p[2 * c], p[2 * c + 1], None, cfg, pk) if grad else \
                ops.conv2d_infer(feats, p[2 * c], p[2 * c + 1], None, cfg, None, pk[:2])
            if c < 4:
                feats = torch.cat((feats, y), 1)
        u = axpby(y, u, RS) if grad else ops._axpby(y, u, RS, 1.0)
    return axpby(u, x, RS) if grad else ops._axpby(u, x, RS, 1.0)


def block():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import esrgan_ref as E
    import rdn_ref as R
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    print("precision mode %s: training forward on %d MFMAs a product, backward on %d, inference on %d"
          % (ops.get_precision(), ops.dense_terms("train_fwd"), ops.dense_terms("bwd"), ops.dense_terms("infer")), flush=True)
    shape, f, g = (16, 64, 32, 32), 64, 32
    rrdb = tuple(tuple(t.to(dev).requires_grad_(True) for t in p) for p in E.make_blocks(f, g, 1, 11)[0])
    params = [t for p in rrdb for t in p]
    x = R.rand(shape, 5).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = R.rand(shape, 6).to(dev).contiguous(memory_format=torch.channels_last)
    packed = [[(ops.pack_weight_fwd(p[2 * c].detach(), False, 0), p[2 * c + 1], ops.pack_weight_bwd(p[2 * c].detach(), False, 0))
               for c in range(5)] for p in rrdb]
    leaves = [x] + params
    axpby = _axpby_fn(ops)

    def fused_fwd():
        with torch.no_grad():
            ops.rrdb_trunk(x, [rrdb], RS)

    def cat_fwd():
        with torch.no_grad():
            _composed_rrdb(ops, x, rrdb, packed, False, axpby)

    def fused():
        torch.autograd.grad(ops.rrdb_trunk(x, [rrdb], RS), leaves, gy)

    def composed():
        torch.autograd.grad(_composed_rrdb(ops, x, rrdb, packed, True, axpby), leaves, gy)

    with torch.no_grad():
        ya, yb = ops.rrdb_trunk(x, [rrdb], RS), _composed_rrdb(ops, x, rrdb, packed, False, axpby)
    a = torch.autograd.grad(ops.rrdb_trunk(x, [rrdb], RS), leaves, gy)
    b = torch.autograd.grad(_composed_rrdb(ops, x, rrdb, packed, True, axpby), leaves, gy)
    print("the two paths compared: outputs apart by %.1e of their maximum, gradients by at most %.1e of theirs"
          % (float((ya - yb).abs().max() / yb.abs().max()),
             max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))), flush=True)
    del a, b
    graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in
              (("fused fwd", fused_fwd), ("cat fwd", cat_fwd), ("fused", fused), ("cat", composed))}
    r = _compare(graphs, 20)
    P = shape[0] * shape[2] * shape[3]
    flop = 2.0 * P * 9 * 3 * (sum((f + c * g) * g for c in range(4)) + (f + 4 * g) * f)
    tag = "x".join(map(str, shape)) + " F=64 G=32"
    print("%s one RRDB forward          slices %s | cat + conv2d + axpby %s = %.2f x the slice path | %.1f TFLOP/s"
          % (tag, _fmt(r["fused fwd"]), _fmt(r["cat fwd"]), r["cat fwd"][0] / r["fused fwd"][0],
             flop / (r["fused fwd"][0] * 1e-3) / 1e12), flush=True)
    print("%s one RRDB forward+backward slices %s | cat + conv2d + axpby %s = %.2f x the slice path | %.1f TFLOP/s"
          % (tag, _fmt(r["fused"]), _fmt(r["cat"]), r["cat"][0] / r["fused"][0], 3 * flop / (r["fused"][0] * 1e-3) / 1e12),
          flush=True)
    for gr in graphs.values():
        gr.close()


def ragan():
    import torch
    import torch.nn.functional as F
    import __graft_entry__
    __graft_entry__.build()
    import esrgan_ref as E
    from pytorch_super_resolution_model_collection_amd import ops, trainers
    dev = torch.device("cuda", 0)
    real, fake = (t.to(dev).requires_grad_(True) for t in E.RAGAN_CASES["B16"])
    for mode in (False, True):
        def fused():
            loss = ops.ragan_loss(real, fake, mode)
            real.grad = fake.grad = None
            ops.backward(loss)

        def composed():
            a, b = real - fake.mean(), fake - real.mean()
            loss = 0.5 * ((F.softplus(a).mean() + F.softplus(-b).mean()) if mode else (F.softplus(-a).mean() + F.softplus(b).mean()))
            real.grad = fake.grad = None
            loss.backward()

        fused()
        ga = (real.grad.clone(), fake.grad.clone())
        composed()
        diff = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(ga, (real.grad, fake.grad)))
        graphs = {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in (("fused", fused), ("torch", composed))}
        r = _compare(graphs, 20)
        print("ragan_loss B = 16 %s forward+backward: one kernel %s | torch composition %s = %.2f x | gradients apart by %.1e"
              % ("G" if mode else "D", _fmt(r["fused"]), _fmt(r["torch"]), r["torch"][0] / r["fused"][0], diff), flush=True)
        for gr in graphs.values():
            gr.close()


def step(nb):
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import perceptual_ref as P
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((16, 3, 32, 32), generator=gen).to(dev), torch.rand((16, 3, 128, 128), generator=gen).to(dev)
    G, D = pkg.RRDBNet(3, 64, nb, 32, 4), pkg.ESRGANDiscriminator(3, 64, 128)
    fill.fill_module(G, 3, 0.3)
    fill.fill_module(D, 4, 1.0)
    G.to(dev).train()
    D.to(dev).train()
    fe = pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, 78)[2]).to(dev)
    g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-5)
    d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-5)
    pre = pkg.trainers.capture_step(pkg.trainers.l1_step(G, g_opt), (inp, tgt), warmup=2, flats=[g_flat])
    adv = pkg.trainers.capture_step(pkg.trainers.esrgan_step(G, D, g_opt, d_opt, fe), (inp, tgt), warmup=2, flats=[g_flat, d_flat])
    r = _compare({"pretrain": lambda: pre(*pre.static), "adversarial": lambda: adv(*adv.static)}, 5)
    print("ESRGAN x4, nb = %d, 16 x 3 x 32 x 32 -> 128 x 128, replayed graphs: L1 pre-training step %9.3f ms (rounds %.3f .. "
          "%.3f) | adversarial step %9.3f ms (rounds %.3f .. %.3f)" % ((nb,) + r["pretrain"] + r["adversarial"]), flush=True)
    torch.cuda.synchronize()
    pre.close()
    adv.close()


def parity():
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-s", "tests/test_ragan_gpu.py", "tests/test_rrdb_gpu.py",
           "tests/test_esrgan_gpu.py"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    for line in r.stdout.splitlines():
        line = line.lstrip(".")
        if "of max |ref|" in line or "oracle" in line or " passed" in line or " failed" in line:
            print(line, flush=True)
    return r.returncode


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
        step(int(sys.argv[2]))
    elif mode == "parity":
        sys.exit(parity())
    else:
        {"block": block, "ragan": ragan}[mode]()
