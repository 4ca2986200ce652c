#!/usr/bin/env python3
"""Evidence for DESIGN 31 (Real-ESRGAN's U-Net discriminator), run on the MI355X box from the repo root:

  python tools/time_realesrgan.py sn        ops.spectral_norm forward + backward at [512, 256, 4, 4] and [64, 64, 3, 3] and the
                                            eight-layer call of the F = 64 net, against the torch composition (mv, normalize,
                                            dot, divide under autograd) it replaces
  python tools/time_realesrgan.py bilinear  ops.upsample_bilinear2x forward + backward at [16, 64, 64, 64] and
                                            [16, 512, 16, 16] (N, C, H, W; channels_last) against F.interpolate
  python tools/time_realesrgan.py loss      ops.gan_logit_loss forward + backward at 16 x 1 x 128 x 128 against softplus().mean()
  python tools/time_realesrgan.py disc      UNetDiscriminatorSN(3, 64) and ESRGANDiscriminator(3, 64, 128) forward + backward
                                            at [16, 3, 128, 128], and the conv kernel every U-Net layer's forward lands on
  python tools/time_realesrgan.py step D NB one replayed ESRGAN adversarial step (batch 16, 32 x 32 LR, 128 x 128 HR, NB blocks)
                                            with discriminator D = vgg (ragan, the default flags) or unet (vanilla)
  python tools/time_realesrgan.py count D   four eager forward + backward passes of discriminator D and nothing else: the
                                            workload of a kernel trace that counts launches (calls / 4)
  python tools/time_realesrgan.py parity    the new GPU tests with their printed errors (worst error over max |fp64 ref|)
  python tools/time_realesrgan.py all       each of the above but `count` as a child process under a time limit of its own,
                                            stopping at the first that fails

HIP events; medians over five alternating rounds of 20 timed replays (steps: 5) each, with the min and max of the round
medians.  Both sides of every comparison are replayed graphs in the same process.  "floor": the bytes the operator has to
move (each operand read once, each result written once) over 6.3 TB/s, the bandwidth a streaming kernel reaches here."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHILD_LIMITS = (("parity", 300), ("sn", 150), ("bilinear", 100), ("loss", 100), ("disc", 150), ("step vgg 2", 200),
                ("step unet 2", 200))
STREAM = 6.3e12


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


def _graphs(sides):
    from pytorch_super_resolution_model_collection_amd import trainers
    return {k: trainers.GraphedFn(fn, (), warmup=2) for k, fn in sides}


def _setup():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    return torch, torch.device("cuda", 0)


def unet_shapes(f=64):
    return [(2 * f, f, 4, 4), (4 * f, 2 * f, 4, 4), (8 * f, 4 * f, 4, 4), (4 * f, 8 * f, 3, 3), (2 * f, 4 * f, 3, 3),
            (f, 2 * f, 3, 3), (f, f, 3, 3), (f, f, 3, 3)]


def sn():
    torch, dev = _setup()
    import torch.nn.functional as F
    import realesrgan_ref as RR
    from pytorch_super_resolution_model_collection_amd import ops
    for tag, shapes in (("[512, 256, 4, 4]", [(512, 256, 4, 4)]), ("[64, 64, 3, 3]", [(64, 64, 3, 3)]),
                        ("the eight layers of F = 64", unet_shapes())):
        cases = [RR.sn_case(s, 40 + i) for i, s in enumerate(shapes)]
        W = [c[0].to(dev).requires_grad_(True) for c in cases]
        G = [RR.randn(s, 70 + i).to(dev) for i, s in enumerate(shapes)]
        ua, va = [c[1].to(dev).clone() for c in cases], [c[2].to(dev).clone() for c in cases]
        ub, vb = [c[1].to(dev).clone() for c in cases], [c[2].to(dev).clone() for c in cases]

        def fused():
            torch.autograd.grad(ops.spectral_norm(list(zip(W, ua, va)), True), W, G)

        def composed():
            outs = []
            for w, u, v in zip(W, ub, vb):
                wm = w.reshape(w.shape[0], -1)
                with torch.no_grad():
                    v.copy_(F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12))
                    u.copy_(F.normalize(torch.mv(wm, v), dim=0, eps=1e-12))
                outs.append(w / torch.dot(u.clone(), torch.mv(wm, v.clone())))
            torch.autograd.grad(outs, W, G)

        r = _compare(_graphs((("fused", fused), ("torch", composed))), 20)
        elems = sum(int(torch.Size(s).numel()) for s in shapes)
        floor = 5 * 4 * elems / STREAM            # forward: W in, w_sn out; backward: G and w_sn in, dW out
        print("spectral_norm %s forward+backward (%d + %d launches): fused %s | torch composition %s = %.2f x | floor %.1f us "
              "= %.1f %% of the fused time" % (tag, 3, 2 * len(shapes), _fmt(r["fused"]), _fmt(r["torch"]),
                                               r["torch"][0] / r["fused"][0], 1e6 * floor, 100 * floor / (1e-3 * r["fused"][0])),
              flush=True)


def bilinear():
    torch, dev = _setup()
    import torch.nn.functional as F
    import realesrgan_ref as RR
    from pytorch_super_resolution_model_collection_amd import ops
    for n, c, h, w in ((16, 64, 64, 64), (16, 512, 16, 16)):
        x = RR.randn((n, h, w, c), 3).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        s = RR.randn((n, h, w, c), 4).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        g = RR.randn((n, 2 * h, 2 * w, c), 5).to(dev).permute(0, 3, 1, 2)
        sides = (("fused", lambda: torch.autograd.grad(ops.upsample_bilinear2x(x), x, g)),
                 ("torch", lambda: torch.autograd.grad(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), x, g)),
                 ("fused add", lambda: torch.autograd.grad(ops.upsample_bilinear2x(x, s), (x, s), g)),
                 ("torch add", lambda: torch.autograd.grad(F.interpolate(x + s, scale_factor=2, mode="bilinear",
                                                                         align_corners=False), (x, s), g)))
        r = _compare(_graphs(sides), 20)
        floor = 10 * 4 * n * c * h * w / STREAM       # forward 1 in + 4 out, backward 4 in + 1 out
        for a, b, extra in (("fused", "torch", 0), ("fused add", "torch add", 1)):
            fl = floor + extra * 4 * n * c * h * w / STREAM
            print("bilinear2x [%d, %d, %d, %d]%s forward+backward: fused %s | F.interpolate %s = %.2f x | floor %.1f us = %.1f %% "
                  "of the fused time" % (n, c, h, w, " with a skip" if extra else "", _fmt(r[a]), _fmt(r[b]),
                                         r[b][0] / r[a][0], 1e6 * fl, 100 * fl / (1e-3 * r[a][0])), flush=True)


def loss():
    torch, dev = _setup()
    import torch.nn.functional as F
    import realesrgan_ref as RR
    from pytorch_super_resolution_model_collection_amd import ops
    x = RR.randn((16, 1, 128, 128), 8, 2.0).to(dev).requires_grad_(True)
    for real in (True, False):
        def fused():
            x.grad = None
            ops.backward(ops.gan_logit_loss(x, real))

        def composed():
            x.grad = None
            (F.softplus(-x) if real else F.softplus(x)).mean().backward()

        r = _compare(_graphs((("fused", fused), ("torch", composed))), 20)
        floor = 8.0 * x.numel() / STREAM
        print("gan_logit_loss 16 x 1 x 128 x 128 %s forward+backward (2 launches): fused %s | torch composition %s = %.2f x | floor "
              "%.2f us = %.1f %% of the fused time" % ("real" if real else "fake", _fmt(r["fused"]), _fmt(r["torch"]),
                                                        r["torch"][0] / r["fused"][0], 1e6 * floor,
                                                        100 * floor / (1e-3 * r["fused"][0])), flush=True)


def _discriminator(pkg, kind, dev):
    import realesrgan_ref as RR
    from oracle import fill
    if kind == "unet":
        D = RR.fill_discriminator(pkg.UNetDiscriminatorSN(3, 64), 4)
    else:
        D = pkg.ESRGANDiscriminator(3, 64, 128)
        fill.fill_module(D, 4, 1.0)
    return D.to(dev).train()


def disc():
    torch, dev = _setup()
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd._lib import ACT_LRELU
    lib = pkg._lib.load()
    gen = torch.Generator().manual_seed(9)
    x = torch.rand((16, 3, 128, 128), generator=gen).to(dev).requires_grad_(True)
    nets = {k: _discriminator(pkg, k, dev) for k in ("unet", "vgg")}
    flats = {k: pkg.optim.FlatParams(d) for k, d in nets.items()}

    def run(kind):
        def fn():
            flats[kind].zero_grad()
            pkg.ops.backward(pkg.ops.gan_logit_loss(nets[kind](x), True))
        return fn

    r = _compare(_graphs((("unet", run("unet")), ("vgg", run("vgg")))), 10)
    print("discriminator forward+backward at [16, 3, 128, 128] (vanilla loss on the logits, gradients into the flat buffer): "
          "UNetDiscriminatorSN(3, 64) %s | ESRGANDiscriminator(3, 64, 128) %s" % (_fmt(r["unet"]), _fmt(r["vgg"])), flush=True)
    # the conv kernel of every U-Net layer's training forward
    D = nets["unet"]
    with torch.no_grad():
        w = pkg.ops.spectral_norm([getattr(D, n).spectral_layer() for n in D.SN_LAYERS], True)
    maps = {"conv0": (3, 128), "conv1": (64, 128), "conv2": (128, 64), "conv3": (256, 32), "conv4": (512, 32), "conv5": (256, 64),
            "conv6": (128, 128), "conv7": (64, 128), "conv8": (64, 128), "conv9": (64, 128)}
    for i, (name, (cin, hw)) in enumerate(maps.items()):
        inp = torch.rand((16, hw, hw, cin), generator=gen).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        layer = getattr(D, name)
        if name in D.SN_LAYERS:
            y = layer.run(inp, w[i - 1].requires_grad_(True), act=ACT_LRELU, slope=0.2)
        else:
            y = layer.run(inp, act=ACT_LRELU, slope=0.2) if name == "conv0" else layer.run(inp)
        fwd = lib.srk_last_kernel_name().decode()
        print("  %s %3d -> %3d, %dx%d, stride %d at %d x %d: forward %s%s"
              % (name, cin, y.shape[1], layer.kernel_size[0], layer.kernel_size[1], layer._s, hw, hw, fwd,
                 "   <== k_conv_generic" if "generic" in fwd else ""), flush=True)


def _step_parts(kind, nb):
    torch, dev = _setup()
    import perceptual_ref as P
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((16, 3, 32, 32), generator=gen).to(dev), torch.rand((16, 3, 128, 128), generator=gen).to(dev)
    G = pkg.RRDBNet(3, 64, nb, 32, 4)
    fill.fill_module(G, 3, 0.3)
    G.to(dev).train()
    D = _discriminator(pkg, kind, dev)
    fe = pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, 78)[2]).to(dev)
    g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-5)
    d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-5)
    step = pkg.trainers.esrgan_step(G, D, g_opt, d_opt, fe, gan_type="vanilla" if kind == "unet" else "ragan")
    return torch, pkg, step, (inp, tgt), [g_flat, d_flat]


def step(kind, nb):
    torch, pkg, eager, batch, flats = _step_parts(kind, nb)
    adv = pkg.trainers.capture_step(eager, batch, warmup=2, flats=flats)
    r = _compare({"adversarial": lambda: adv(*adv.static)}, 5)
    print("ESRGAN x4, nb = %d, 16 x 3 x 32 x 32 -> 128 x 128, --discriminator %s, replayed graph: adversarial step %9.3f ms "
          "(rounds %.3f .. %.3f)" % ((nb, kind) + r["adversarial"]), flush=True)
    torch.cuda.synchronize()
    adv.close()


def count(kind):
    torch, dev = _setup()
    import pytorch_super_resolution_model_collection_amd as pkg
    D = _discriminator(pkg, kind, dev)
    flat = pkg.optim.FlatParams(D)
    x = torch.rand((16, 3, 128, 128), generator=torch.Generator().manual_seed(9)).to(dev).requires_grad_(True)
    for _ in range(4):
        flat.zero_grad()
        pkg.ops.backward(pkg.ops.gan_logit_loss(D(x), True))
    torch.cuda.synchronize()
    print("four forward + backward passes of the %s discriminator done" % kind, flush=True)


def parity():
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-s", "tests/test_realesrgan_gpu.py"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    for line in r.stdout.splitlines():
        line = line.lstrip(".")
        if "of max |ref|" in line or "oracle" in line or " passed" in line or " failed" in line or "gan_logit_loss n=" in line:
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
        step(sys.argv[2], int(sys.argv[3]))
    elif mode == "count":
        count(sys.argv[2])
    elif mode == "parity":
        sys.exit(parity())
    else:
        {"sn": sn, "bilinear": bilinear, "loss": loss, "disc": disc}[mode]()
