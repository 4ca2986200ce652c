#!/usr/bin/env python3
"""Evidence for DESIGN 21 (the perceptual loss that trains), run on the MI355X box from the repo root:

  python tools/time_perceptual.py pool     ops.max_pool2x2_train forward + backward (k_maxpool2 + k_maxpool2_bwd) against
                                           ATen's max_pool2d forward + backward on the device at [16, 64, 128, 128], both
                                           channels_last (ATen saves an index tensor; ours recomputes the winners)
  python tools/time_perceptual.py term     ops.perceptual_loss forward + backward at [16, 3, 128, 128] (features[:9]), and
                                           the target's half alone (what the logged term already paid twice)
  python tools/time_perceptual.py step     one replayed c5-shaped SRGAN step (16 x 3 x 32 x 32 -> 128 x 128, G(3,64,16),
                                           D(3,64,128)): without an extractor, with the logged term, with perceptual=True
  python tools/time_perceptual.py parity   the case table of tests/test_perceptual_gpu.py against float64: error of the
                                           device, of torch's fp32 CPU evaluation, the contract and the bar used

HIP events; medians over five alternating rounds of 30 timed calls (steps: 20) each, with the spread of the round medians."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def _setup():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    return torch, pkg, torch.device("cuda", 0)


def _fmt(r):
    return "%8.3f ms (rounds %.3f .. %.3f)" % r


def pool():
    torch, pkg, dev = _setup()
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(5)
    shape = (16, 64, 128, 128)
    x = torch.randn(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn((16, 64, 64, 64), generator=gen).to(dev).contiguous(memory_format=torch.channels_last)

    def ours():
        x.grad = None
        pkg.ops.max_pool2x2_train(x).backward(dy)

    def aten():
        x.grad = None
        F.max_pool2d(x, 2, 2).backward(dy)

    def ours_fwd():
        with torch.no_grad():
            pkg.ops.max_pool2x2(x)
    ours()
    a = x.grad.clone()
    aten()
    same = torch.equal(a, x.grad)
    r = _compare({"ours": ours, "aten": aten, "fwd": ours_fwd}, 30)
    nbytes = 4 * (x.numel() * 2 + dy.numel())       # backward: reads x and dy, writes dx
    bwd = r["ours"][0] - r["fwd"][0]
    print("%s pool fwd+bwd: ours %s, forward alone %s -> backward ~%.3f ms = %.0f GB/s of its %d MB | ATen %s = %.2f x ours | "
          "gradients bit-equal: %s" % ("x".join(map(str, shape)), _fmt(r["ours"]), _fmt(r["fwd"]), bwd,
                                       nbytes / bwd / 1e6, nbytes >> 20, _fmt(r["aten"]), r["aten"][0] / r["ours"][0], same),
          flush=True)


def _head(pkg, dev, seed=78):
    import perceptual_ref as P
    return pkg.FeatureExtractor().load_vgg19(P.filled_head(8, seed)[2]).to(dev)


def term():
    torch, pkg, dev = _setup()
    fe = _head(pkg, dev)
    gen = torch.Generator().manual_seed(6)
    shape = (16, 3, 128, 128)
    t = torch.rand(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    x = (t + 0.05 * torch.randn(shape, generator=gen).to(dev)).contiguous(memory_format=torch.channels_last).requires_grad_(True)

    def full():
        x.grad = None
        with pkg.ops.premasked_gradients():
            pkg.ops.backward(pkg.ops.perceptual_loss(x, t, fe))

    def plain_protocol():
        x.grad = None
        pkg.ops.backward(pkg.ops.perceptual_loss(x, t, fe))

    def logged():
        with torch.no_grad():
            pkg.ops.mse_loss(fe(pkg.utils.norm(x.detach(), vgg=True)), fe(pkg.utils.norm(t, vgg=True)))
    r = _compare({"full": full, "plain": plain_protocol, "logged": logged}, 30)
    print("%s perceptual_loss (features[:9]) fwd+bwd, pre-masked gradients as in a train step %s | standard protocol %s | "
          "the detached, logged term (two no-grad forwards + MSE) %s" % ("x".join(map(str, shape)), _fmt(r["full"]),
                                                                     _fmt(r["plain"]), _fmt(r["logged"])), flush=True)


def step():
    torch, pkg, dev = _setup()
    gen = torch.Generator().manual_seed(1234)
    lr_img = torch.rand(16, 3, 32, 32, generator=gen).to(dev)
    hr_img = torch.rand(16, 3, 128, 128, generator=gen).to(dev)
    fe = _head(pkg, dev)
    steps = {}
    for name, kw in (("no extractor", {}), ("logged term", {"feature_extractor": fe}),
                     ("perceptual", {"feature_extractor": fe, "perceptual": True})):
        G, D = pkg.SRGANGenerator(3, 64, 16), pkg.SRGANDiscriminator(3, 64, 128)
        torch.manual_seed(1234)
        G.weight_init()
        D.weight_init()
        G.to(dev).train()
        D.to(dev).train()
        gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-4)
        d_opt = pkg.optim.make_optimizer("srgan_d", dflat, 1e-4)
        eager = pkg.trainers.srgan_step(G, D, g_opt, d_opt, lazy_pack=True, **kw)
        steps[name] = (pkg.trainers.GraphedFn(eager, (lr_img, hr_img), flats=[gflat, dflat]), G, D, g_opt, d_opt)
    r = _compare({k: (lambda s=s: s[0](lr_img, hr_img)) for k, s in steps.items()}, 20)
    base = r["no extractor"][0]
    print("c5-shaped SRGAN step, replayed graph: no extractor %s | logged term %s (+%.3f ms) | perceptual=True %s (+%.3f ms "
          "= %.1f %%)" % (_fmt(r["no extractor"]), _fmt(r["logged term"]), r["logged term"][0] - base, _fmt(r["perceptual"]),
                          r["perceptual"][0] - base, (r["perceptual"][0] / base - 1) * 100), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def parity():
    torch, pkg, dev = _setup()
    import perceptual_ref as P
    row = "%-34s max|ref| %.4e  device err %.3e  torch fp32 CPU err %.3e  contract %.3e  bar %.3e  %s"

    def line(what, got, ref, contract, err32):
        err, scale = P.max_err(got, ref)
        bound = P.bar(contract, err32, scale)
        print(row % (what, scale, err, err32, contract * scale, bound, "ok" if err <= bound else "MISSES"), flush=True)
    for fl, shape in P.HEAD_CASES:
        fe = pkg.FeatureExtractor(feature_layer=fl).load_vgg19(P.filled_head(fl)[2]).to(dev)
        case = P.head_case(fl, shape)
        x = case["x"].to(dev).requires_grad_(True)
        f = fe.extract(x, grad=True)
        (f * case["g"].to(dev)).sum().backward()
        tag = "layer %d %s " % (fl, "x".join(map(str, shape)))
        line(tag + "features", f, case["f64"], P.OUT_CONTRACT, case["f_err32"])
        line(tag + "dx", x.grad, case["dx64"], P.GRAD_CONTRACT, case["dx_err32"])
    fe = pkg.FeatureExtractor().load_vgg19(P.filled_head(8)[2]).to(dev)
    for shape in P.LOSS_SHAPES:
        case = P.loss_case(shape)
        for premask in (False, True):
            p = case["pred"].to(dev).requires_grad_(True)
            loss = pkg.ops.perceptual_loss(p, case["target"].to(dev), fe)
            if premask:
                with pkg.ops.premasked_gradients():
                    loss.backward()
            else:
                loss.backward()
            tag = "loss %s %s" % ("x".join(map(str, shape)), "premasked " if premask else "")
            line(tag + "value", loss.reshape(1), torch.tensor([case["l64"]], dtype=torch.float64), P.OUT_CONTRACT, case["l_err32"])
            line(tag + "d/dpred", p.grad, case["d64"], P.GRAD_CONTRACT, case["d_err32"])


if __name__ == "__main__":
    {"pool": pool, "term": term, "step": step, "parity": parity}[sys.argv[1]]()
