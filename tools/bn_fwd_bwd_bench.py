#!/usr/bin/env python3
"""Time one BatchNorm forward + backward (ops.batch_norm, training) at [16, 64, 96, 96] with device events, in four arms:
ops.BN_FIN_APPLY True / False x no activation / LeakyReLU.  An eager loop: six launches of ~10 us per iteration, so the
host's pace shows in the numbers (profiles/bn_refactor_ab.txt).  The False arms are the separate launches (k_bn_reduce16, the
float4 backward apply), which the SRGAN step of bench.py never reaches.
   python tools/bn_fwd_bwd_bench.py [iters] [checkout]     (checkout: the tree whose package is timed; default this one)"""
import os, sys, torch
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_super_resolution_model_collection_amd as pkg
ops, dev = pkg.ops, torch.device("cuda:0")
n, c, h, w = 16, 64, 96, 96
torch.manual_seed(1234)
x = torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
dy = torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last)
gamma, beta = torch.rand(c, device=dev).add_(0.5).requires_grad_(True), torch.randn(c, device=dev).requires_grad_(True)
rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)


def once(act):
    y = ops.batch_norm(x, gamma, beta, rm, rv, True, 0.1, 1e-5, None, None, act, 0.2)
    y.backward(dy)
    x.grad = gamma.grad = beta.grad = None


for fin in (True, False):
    ops.BN_FIN_APPLY = fin
    for name, act in (("none", pkg._lib.ACT_NONE), ("lrelu", pkg._lib.ACT_LRELU)):
        for _ in range(20):
            once(act)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            once(act)
        e1.record()
        torch.cuda.synchronize()
        print("bn fwd+bwd 16x64x96x96 fin=%d act=%s: %.4f ms" % (fin, name, e0.elapsed_time(e1) / iters))
