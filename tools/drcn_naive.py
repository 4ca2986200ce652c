"""DRCN's train step composed naively from the package's generic layers: D separate ops.conv2d recursions, the
reconstruction as 2*D separate convolutions, one ops.mse_loss per term and torch arithmetic for the combine and the
weight-decay term.  The yardstick of the fused path (models.DRCNNet + ops.recursive_conv + ops.drcn_head): shared by
tests/test_drcn_gpu.py (same loss and gradients) and tools/time_drcn.py (the step time it saves)."""
import torch

from pytorch_super_resolution_model_collection_amd import ops
from pytorch_super_resolution_model_collection_amd._lib import ACT_RELU


def naive_reconstructions(model, x):
    h = model.embedding_layer(x)
    c = model.conv_block.conv
    cfg = ops.ConvCfg(c._s, c._p, act=ACT_RELU)
    ys = []
    for _ in range(model.num_recursions):
        h = ops.conv2d(h, c.weight, c.bias, None, cfg)
        ys.append(model.reconstruction_layer(h))
    return ys


def naive_loss(model, x, target, alpha, beta):
    """alpha * mean_d MSE(y_d, t) + (1 - alpha) * MSE(out, t) + beta * sum_theta sum theta^2 (drcn.py:203-215)."""
    ys = naive_reconstructions(model, x)
    D = len(ys)
    w = model.w
    loss1 = 0
    for y in ys:
        loss1 = loss1 + ops.mse_loss(y, target) / D
    acc = 0
    for d, y in enumerate(ys):
        acc = acc + y * w[d]
    out = (acc * (1.0 / torch.sum(w)) + x).contiguous(memory_format=torch.channels_last)
    loss2 = ops.mse_loss(out, target)
    reg = 0
    for p in model.parameters():
        reg = reg + torch.sum(p ** 2)
    return alpha * loss1 + (1 - alpha) * loss2 + beta * reg
