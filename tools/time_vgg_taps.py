#!/usr/bin/env python3
"""Evidence for DESIGN 33 (the multi-layer VGG feature loss), run on the MI355X box from the repo root:

  python tools/time_vgg_taps.py op      ops.vgg_tap, forward and forward + backward, at the five taps of a [16, 3, 128, 128]
                                        batch, against the composition of the operators the package had before (ops.fork,
                                        ops.l1_loss, a ReLU launch, ops.max_pool2x2_train; the target's ReLU and pool
                                        without a graph), each as a share of its HBM bound from the bytes its shapes say
  python tools/time_vgg_taps.py term    the whole term ops.vgg_feature_loss at [16, 3, 128, 128], forward + backward, fused
                                        against tests/vgg_taps_ref.composition, and what is left of it after the five taps
                                        (the VGG convs, two normalisations and the finish)
  python tools/time_vgg_taps.py step    one replayed ESRGAN step, nb = 2, batch 16, 32 x 32 LR, --discriminator unet
                                        --gan_type vanilla: vgg_layers = realesrgan against the single conv5_4 tap
  python tools/time_vgg_taps.py default [ROUNDS]   the default-flag step alone, its median (for an A/B of two checkouts on
                                        one box: run it from either tree in turn)
  python tools/time_vgg_taps.py all     op, term and step as child processes under time limits of their own, stopping at
                                        the first that fails

HIP events; medians over five alternating rounds of `inner` timed replays each, with the lowest and highest round.  The HBM
bound uses 6.3 TB/s, the bandwidth a streaming kernel reaches on this part.  The largest pair of maps is 134 MB and fits the
256 MB last-level cache, as DESIGN 21 notes for the pool: a replayed tap may be served from it, and where a figure is above
100 % of the bound it is not an HBM figure; the tool says so."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BATCH = (16, 3, 128, 128)
TAPS = (((16, 64, 128, 128), "pool"), ((16, 128, 64, 64), "pool"), ((16, 256, 32, 32), "pool"), ((16, 512, 16, 16), "pool"),
        ((16, 512, 8, 8), "last"))
HBM_BYTES_PER_S = 6.3e12
CHILD_LIMITS = (("op", 200), ("term", 150), ("step", 240))


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


def _bound_note(maps, numel, got_ms):
    bound_ms = maps * numel * 4 / HBM_BYTES_PER_S * 1e3
    pct = 100.0 * bound_ms / got_ms
    return "%.2f maps = %.2f us at the HBM bound, %.0f %% of it%s" % (
        maps, 1e3 * bound_ms, pct, " (above it: served from the last-level cache, not an HBM figure)" if pct > 100 else "")


def _tap_sides(torch, pkg, dev, shape, mode_name, gen):
    """{name: fn} for one tap: fused and composed, forward alone and forward + backward."""
    ops, L = pkg.ops, pkg._lib
    mode = {"pool": L.VGG_TAP_POOL, "relu": L.VGG_TAP_RELU, "last": L.VGG_TAP_LAST}[mode_name]
    cl = lambda: torch.randn(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    a, b = cl().requires_grad_(True), cl()
    n, c, h, w = shape
    gy = None if mode == L.VGG_TAP_LAST else torch.randn((n, c, h // 2, w // 2), generator=gen).to(dev).contiguous(
        memory_format=torch.channels_last)
    ws = torch.empty(int(L.load().srk_vgg_tap_workspace_bytes(1)), dtype=torch.uint8, device=dev)
    unit = ops.unit_seed(dev)

    def fused_graph():
        token, ya, yb = ops.vgg_tap(a, b, mode, 1.0, 0, 1, ws)
        return ops.vgg_tap_finish(ws, 1, [token]), ya

    def composed_graph():
        if mode == L.VGG_TAP_LAST:
            return ops.l1_loss(a, b), None
        keep, t = ops.fork(a)
        loss = ops.l1_loss(keep, b)
        ya = ops.max_pool2x2_train(ops.activation(t, L.ACT_RELU))
        with torch.no_grad():
            ops.max_pool2x2(ops.activation(b, L.ACT_RELU))
        return loss, ya

    def fwd(build):
        def run():
            with torch.no_grad():
                build()
        return run

    def both(build):
        def run():
            loss, ya = build()
            outs, grads = ([loss], [unit]) if ya is None else ([loss, ya], [unit, gy])
            torch.autograd.grad(outs, a, grads)
        return run

    # the two sides compute the same thing: checked once before anything is timed
    lf, yf = fused_graph()
    lc, yc = composed_graph()
    gf = torch.autograd.grad([lf] + ([] if yf is None else [yf]), a, [unit] + ([] if yf is None else [gy]))[0]
    gc = torch.autograd.grad([lc] + ([] if yc is None else [yc]), a, [unit] + ([] if yc is None else [gy]))[0]
    assert yf is None or torch.equal(yf, yc)
    diff = float((gf - gc).abs().max() / gc.abs().max())
    assert diff < 1e-5 and abs(float(lf) - float(lc)) < 1e-5 * abs(float(lc)), (diff, float(lf), float(lc))
    return {"fused fwd": fwd(fused_graph), "composed fwd": fwd(composed_graph), "fused": both(fused_graph),
            "composed": both(composed_graph)}, a.numel(), mode == L.VGG_TAP_LAST


def op():
    torch, pkg, dev = _setup()
    gen = torch.Generator().manual_seed(5)
    for shape, mode in TAPS:
        sides, numel, last = _tap_sides(torch, pkg, dev, shape, mode, gen)
        graphs = {k: pkg.trainers.GraphedFn(fn, (), warmup=2) for k, fn in sides.items()}
        r = _compare(graphs, 20)
        name = "%s %s" % ("x".join(map(str, shape)), mode.upper())
        print("%-22s forward          fused %s | composition %s = %.2f x the fused tap | %s"
              % (name, _fmt(r["fused fwd"]), _fmt(r["composed fwd"]), r["composed fwd"][0] / r["fused fwd"][0],
                 _bound_note(2.0 if last else 2.5, numel, r["fused fwd"][0])), flush=True)
        print("%-22s forward+backward fused %s | composition %s = %.2f x the fused tap | %s"
              % (name, _fmt(r["fused"]), _fmt(r["composed"]), r["composed"][0] / r["fused"][0],
                 _bound_note(5.0 if last else 5.75, numel, r["fused"][0])), flush=True)
        for g in graphs.values():
            g.close()


def _extractor(pkg, dev):
    import perceptual_ref as P
    return pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, 78)[2]).to(dev)


def term():
    torch, pkg, dev = _setup()
    import vgg_taps_ref as R
    ops = pkg.ops
    fe = _extractor(pkg, dev)
    gen = torch.Generator().manual_seed(6)
    pred = torch.rand(BATCH, generator=gen).to(dev).requires_grad_(True)
    target = torch.rand(BATCH, generator=gen).to(dev)
    layers = dict(ops.REALESRGAN_VGG_LAYERS)

    def fused():
        torch.autograd.grad(ops.vgg_feature_loss(pred, target, fe, layers), pred, ops.unit_seed(dev))

    def composed():
        torch.autograd.grad(R.composition(pkg, fe, pred, target), pred, ops.unit_seed(dev))

    def single():
        torch.autograd.grad(ops.perceptual_loss(pred, target, fe, criterion='l1'), pred, ops.unit_seed(dev))

    graphs = {k: pkg.trainers.GraphedFn(fn, (), warmup=2) for k, fn in (("fused", fused), ("composed", composed),
                                                                       ("single", single))}
    r = _compare(graphs, 5)
    print("the term at %s, forward + backward, replayed: fused %s | composition %s = %.3f x the fused term | the single "
          "conv5_4 tap (ops.perceptual_loss) %s" % ("x".join(map(str, BATCH)), _fmt(r["fused"]), _fmt(r["composed"]),
                                                    r["composed"][0] / r["fused"][0], _fmt(r["single"])), flush=True)
    for g in graphs.values():
        g.close()
    gen = torch.Generator().manual_seed(5)
    taps_f = taps_c = 0.0
    for shape, mode in TAPS:
        sides, _, _ = _tap_sides(torch, pkg, dev, shape, mode, gen)
        graphs = {k: pkg.trainers.GraphedFn(sides[k], (), warmup=2) for k in ("fused", "composed")}
        rr = _compare(graphs, 20, rounds=3)
        taps_f, taps_c = taps_f + rr["fused"][0], taps_c + rr["composed"][0]
        for g in graphs.values():
            g.close()
    print("its five taps alone, forward + backward: fused %.2f us, composition %.2f us; the rest of the fused term (both "
          "operands' 16 VGG convs, the pred's data gradients, two normalisations, the finish) %.2f us = %.1f %% of it"
          % (1e3 * taps_f, 1e3 * taps_c, 1e3 * (r["fused"][0] - taps_f), 100.0 * (1.0 - taps_f / r["fused"][0])), flush=True)


def _esrgan_step(torch, pkg, dev, vgg_layers):
    from oracle import fill
    G, D = pkg.RRDBNet(3, 64, 2, 32, 4), pkg.UNetDiscriminatorSN(3, 64)
    fill.fill_module(G, 5, 0.7)
    G.to(dev).train()
    D.to(dev).train()
    g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-4)
    d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-4)
    kw = {} if vgg_layers is None else {"vgg_layers": vgg_layers}
    step = pkg.trainers.esrgan_step(G, D, g_opt, d_opt, _extractor(pkg, dev), gan_type="vanilla", **kw)
    gen = torch.Generator().manual_seed(9)
    batch = (torch.rand((16, 3, 32, 32), generator=gen).to(dev), torch.rand((16, 3, 128, 128), generator=gen).to(dev))
    return pkg.trainers.capture_step(step, batch, warmup=2, flats=[g_flat, d_flat])


def step():
    torch, pkg, dev = _setup()
    torch.manual_seed(0)
    graphs = {"single": _esrgan_step(torch, pkg, dev, None),
              "realesrgan": _esrgan_step(torch, pkg, dev, dict(pkg.ops.REALESRGAN_VGG_LAYERS))}
    r = _compare({k: (lambda g=g: g(*g.static)) for k, g in graphs.items()}, 5)
    s, m = r["single"], r["realesrgan"]
    print("ESRGAN step, nb = 2, 16 x 3 x 32 x 32 -> 128 x 128, U-Net discriminator, vanilla GAN loss, replayed: the single "
          "conv5_4 tap %8.3f ms (rounds %.3f .. %.3f) | vgg_layers = realesrgan %8.3f ms (rounds %.3f .. %.3f) = %.3f x"
          % (s[0], s[1], s[2], m[0], m[1], m[2], m[0] / s[0]), flush=True)
    for g in graphs.values():
        g.close()


def default(rounds=5):
    torch, pkg, dev = _setup()
    torch.manual_seed(0)
    g = _esrgan_step(torch, pkg, dev, None)
    v = [_events(lambda: g(*g.static), 5) for _ in range(int(rounds))]
    print("default-flag ESRGAN step (tree %s): median %.3f ms (rounds %.3f .. %.3f)"
          % (ROOT, statistics.median(v), min(v), max(v)), flush=True)
    g.close()


def main(argv):
    what = argv[0] if argv else "all"
    if what == "all":
        for name, limit in CHILD_LIMITS:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), name], timeout=limit).returncode
            if rc != 0:
                print("time_vgg_taps.py %s ended with status %d: stopping" % (name, rc), flush=True)
                return rc
        return 0
    if what == "default":
        default(*argv[1:2])
        return 0
    {"op": op, "term": term, "step": step}[what]()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
