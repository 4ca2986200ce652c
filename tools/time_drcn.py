#!/usr/bin/env python3
"""DRCN step time at the reference defaults (batch 16, crop 128, C = 3, F = 256, D = 16; drcn.py:103-104): the fused
train step (stacked recursion + fused head, trainers.drcn_step) replayed as a hipGraph, the same step eagerly, the naive
composition (tools/drcn_naive.py: 16 separate recursions, 16 x 2 reconstruction convs, ops.mse_loss terms; eager, torch
Adam), and the 1 x 3 x 512 x 512 eval.  FLOPs from shapes, share of the 3-MFMA peak (833 TF).  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_TF = 833.0


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def conv_flops(n, h, w, cin, cout):
    return 2.0 * n * h * w * cin * cout * 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--naive_steps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from tools.drcn_naive import naive_loss
    ops, optim, trainers = pkg.ops, pkg.optim, pkg.trainers
    dev = torch.device("cuda:0")
    C, Fb, D, n, s = 3, 256, 16, a.batch, a.crop
    torch.manual_seed(0)
    model = pkg.DRCNNet(C, Fb, D)
    model.weight_init()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    flat = optim.FlatParams(model)
    opt = optim.make_optimizer("drcn", flat, 1e-5)
    w_opt = optim.TensorAdam(model.w, 1e-5)
    alpha = torch.tensor(0.96, device=dev)
    step = trainers.drcn_step(model, opt, w_opt, alpha, 1e-3)
    x = torch.rand(n, C, s, s, device=dev).contiguous(memory_format=torch.channels_last)
    t = torch.rand(n, C, s, s, device=dev).contiguous(memory_format=torch.channels_last)
    eager_ms = timed(lambda: step(x, t), 1, 3)
    g = trainers.GraphedFn(step, [x, t], warmup=1, flats=[flat])
    graph_ms = timed(lambda: g(x, t), a.warmup, a.steps)
    loss = float(g.out.detach())
    del g
    torch.cuda.synchronize()
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30

    # the naive composition (its own copy of the weights, autograd gradients, torch Adam)
    base = pkg.DRCNNet(C, Fb, D)
    base.load_state_dict(sd)
    base = base.to(dev).train()
    topt = torch.optim.Adam([{'params': list(base.parameters())}, {'params': [base.w]}], lr=1e-5)

    def naive_step():
        topt.zero_grad()
        lo = naive_loss(base, x, t, 0.96, 1e-3)
        lo.backward()
        topt.step()
        return lo
    naive_ms = timed(naive_step, 1, a.naive_steps)
    del base, topt
    torch.cuda.empty_cache()

    model.eval()
    xe = torch.rand(1, C, 512, 512, device=dev)
    with torch.no_grad():
        eval_ms = timed(lambda: model(xe), 2, 5)

    def fwd_flops(nn, hh, ww):
        f = conv_flops(nn, hh, ww, C, Fb) + conv_flops(nn, hh, ww, Fb, Fb)          # embedding
        f += D * (conv_flops(nn, hh, ww, Fb, Fb)                                   # recursion
                  + conv_flops(nn, hh, ww, Fb, Fb) + conv_flops(nn, hh, ww, Fb, C))  # reconstruction
        return f
    fwd = fwd_flops(n, s, s)
    train_flops = 3 * fwd - conv_flops(n, s, s, C, Fb)    # forward + data + weight gradients (no dx of the input)
    res = {"metric": "drcn_train_step_ms", "batch": n, "crop": s, "C": C, "F": Fb, "D": D,
           "graph_step_ms": round(graph_ms, 3), "eager_step_ms": round(eager_ms, 3), "naive_step_ms": round(naive_ms, 3),
           "speedup_vs_naive": round(naive_ms / graph_ms, 3), "loss": loss,
           "train_tflop": round(train_flops / 1e12, 3), "train_tflops": round(train_flops / graph_ms / 1e9, 1),
           "train_peak_share": round(train_flops / graph_ms / 1e9 / PEAK_TF, 3),
           "eval_512_ms": round(eval_ms, 3), "eval_512_tflop": round(fwd_flops(1, 512, 512) / 1e12, 3),
           "eval_peak_share": round(fwd_flops(1, 512, 512) / eval_ms / 1e9 / PEAK_TF, 3),
           "peak_mem_gb": round(peak_gb, 2), "precision": ops.get_precision()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
