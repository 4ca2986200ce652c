#!/usr/bin/env python3
"""Generates tests/golden/drcn.npz by running the REFERENCE's DRCN (drcn.Net and the loss / optimizer of its train
loop, drcn.py:13-59 and 101-221) on the CPU.

The reference constructor calls `.cuda()` on its combine weights; it is patched to the identity while the net is built
and run.  Two nets (C = 1 and C = 3; F = 16, D = 4; input 2 x C x 20 x 20) with `fill`-seeded parameters and unequal
combine weights.  Stored per net (prefix c1_ / c3_), arrays only:
  inputs x, t; w; every parameter (p_<state_dict key>)
  y (the D reconstructions, [D, N, C, H, W]) and out of the forward pass
  L1 = mean_d MSE(y_d, t), L2 = MSE(out, t), R = sum_theta sum theta^2 and L at each alpha of ALPHAS
  gradients of every parameter (g_<key>) and of w (g_w) of the loss at alpha = GRAD_ALPHA
  parameters (a_<key>) and w (a_w) after three Adam steps (lr ADAM_LR) at alpha = STEP_ALPHAS
  keys: the state_dict keys in order (of the F = 256, D = 16 net the trainer builds)

Run:  python tests/golden/make_golden_drcn.py      (needs the reference checkout of make_golden.REF; CPU only; the output is byte-identical)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden  # noqa: E402
from oracle import fill  # noqa: E402

F, D, N, HW = 16, 4, 2, 20
ALPHAS = (1.0, 0.96, 0.3, 0.0)
GRAD_ALPHA = 0.96
STEP_ALPHAS = (0.96, 0.92, 0.0)
BETA = 1e-3
ADAM_LR = 1e-4


def reference_drcn():
    make_golden.import_reference()
    import drcn
    return drcn


def losses(net, x, t, alpha):
    """drcn.py:203-215, term by term."""
    mse = torch.nn.MSELoss()
    y_d, out = net(x)
    loss1 = 0
    for d in range(net.num_recursions):
        loss1 += mse(y_d[d], t) / net.num_recursions
    loss2 = mse(out, t)
    reg = 0
    for theta in net.parameters():
        reg += torch.mean(torch.sum(theta ** 2))
    return y_d, out, loss1, loss2, reg, alpha * loss1 + (1 - alpha) * loss2 + BETA * reg


def make_net(drcn, c, seed):
    net = drcn.Net(c, F, D)
    fill.fill_module(net, seed=seed)
    with torch.no_grad():
        net.w.copy_(torch.tensor([0.4, 0.15, 0.3, 0.25]) * torch.tensor([1.0, 1.3, 0.7, 1.1]))
    return net


def main():
    drcn = reference_drcn()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        arrays = {}
        arrays["keys"] = np.array(list(drcn.Net(3, 256, 16).state_dict().keys()))
        arrays["keys_shapes"] = np.array([list(v.shape) + [1] * (4 - v.dim())
                                          for v in drcn.Net(3, 256, 16).state_dict().values()], dtype=np.int64)
        for c, seed in ((1, 71), (3, 73)):
            pre = "c%d_" % c
            net = make_net(drcn, c, seed)
            x = fill.rand((N, c, HW, HW), seed + 1)
            t = fill.rand((N, c, HW, HW), seed + 2)
            arrays[pre + "x"], arrays[pre + "t"] = x.numpy(), t.numpy()
            arrays[pre + "w"] = net.w.detach().numpy().copy()
            for k, v in net.state_dict().items():
                arrays[pre + "p_" + k] = v.numpy().copy()
            with torch.no_grad():
                for i, a in enumerate(ALPHAS):
                    y_d, out, l1, l2, reg, loss = losses(net, x, t, a)
                    arrays[pre + "terms_%d" % i] = np.array([a, float(l1), float(l2), float(reg), float(loss)],
                                                            dtype=np.float64)
            arrays[pre + "y"] = torch.stack(y_d).numpy()
            arrays[pre + "out"] = out.numpy()
            # gradients of the loss at GRAD_ALPHA (drcn.py:217)
            net.zero_grad()
            net.w.grad = None
            _, _, _, _, _, loss = losses(net, x, t, GRAD_ALPHA)
            loss.backward()
            for k, p in net.named_parameters():
                arrays[pre + "g_" + k] = p.grad.numpy().copy()
            arrays[pre + "g_w"] = net.w.grad.numpy().copy()
            # three Adam steps of the two param groups (drcn.py:108-111, 216-218)
            opt = torch.optim.Adam([{'params': list(net.parameters())}, {'params': [net.w]}], lr=ADAM_LR)
            for a in STEP_ALPHAS:
                opt.zero_grad()
                _, _, _, _, _, loss = losses(net, x, t, a)
                loss.backward()
                opt.step()
            for k, v in net.state_dict().items():
                arrays[pre + "a_" + k] = v.numpy().copy()
            arrays[pre + "a_w"] = net.w.detach().numpy().copy()
        arrays["alphas"] = np.array(ALPHAS, dtype=np.float64)
        arrays["step_alphas"] = np.array(STEP_ALPHAS, dtype=np.float64)
        arrays["consts"] = np.array([GRAD_ALPHA, BETA, ADAM_LR, F, D], dtype=np.float64)
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "drcn.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(arrays)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
