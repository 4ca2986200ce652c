"""The yardstick of the perceptual (VGG feature) loss tests: the head as stock torch.nn layers in torchvision's vgg19
layout, evaluated in float64 on the CPU with the weights oracle.fill gives it -- features, the loss
MSE(head(norm(pred)), head(norm(target))) and their gradients -- plus the bars the tests hold the device path to.

Bars.  The project's contract is 1e-4 * max|ref| for outputs and 1e-3 * max|ref| for gradients.  A chain of fp32 convs,
ReLUs and pools need not meet that in ANY fp32 evaluation (a ReLU / pool decision flips where the pre-activation is
within rounding of zero / of its neighbour), so each bar is max(contract, 2 * the error of torch's own fp32 CPU
evaluation of the same graph against fp64 on the same inputs) -- the rule the SRGAN step's gradients already live under.
Both numbers are printed by the tests and recorded in profiles/perceptual_parity.txt.

Run as a program (`python tests/perceptual_ref.py dp-child`) it is the child process of the data-parallel step test."""
import copy
import functools
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402

VGG19_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M')
VGG_MEAN, VGG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUT_CONTRACT, GRAD_CONTRACT = 1e-4, 1e-3

# (feature_layer, input shape): the whole table of the head tests
HEAD_CASES = [(8, (2, 3, 12, 10)), (8, (1, 3, 9, 7)), (11, (1, 3, 12, 12)), (11, (1, 3, 10, 10))]
LOSS_SHAPES = [(2, 3, 12, 10), (1, 3, 9, 7)]
POOL_SHAPES = [(1, 5, 7, 9), (2, 8, 6, 10), (1, 64, 2, 2), (1, 4, 3, 2), (1, 3, 2, 3), (1, 1, 5, 5)]


def torch_vgg_head(feature_layer=8):
    """vgg19.features[:feature_layer + 1] from stock torch.nn layers (what torchvision constructs), float32."""
    mods, cin = [], 3
    for v in VGG19_CFG:
        if v == 'M':
            mods.append(nn.MaxPool2d(2, 2))
        else:
            mods += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(False)]
            cin = v
    return nn.Sequential(*mods[:feature_layer + 1])


@functools.lru_cache(maxsize=None)
def filled_head(feature_layer=8, seed=77):
    """(float32 head, its float64 copy, the state_dict under torchvision's `features.` names)."""
    h32 = fill.fill_module(torch_vgg_head(feature_layer), seed)
    h64 = copy.deepcopy(h32).double()
    for p in list(h32.parameters()) + list(h64.parameters()):
        p.requires_grad_(False)
    sd = {"features." + k: v.clone() for k, v in h32.state_dict().items()}
    return h32, h64, sd


def vnorm(t):
    m = torch.tensor(VGG_MEAN, dtype=t.dtype).view(-1, 1, 1)
    s = torch.tensor(VGG_STD, dtype=t.dtype).view(-1, 1, 1)
    return (t - m) / s


def head_eval(head, x, g):
    """(features, d sum(features * g) / dx) of `head` in the dtype of its weights."""
    dt = next(head.parameters()).dtype
    x = x.detach().to(dt).requires_grad_(True)
    f = head(x)
    (f * g.to(dt)).sum().backward()
    return f.detach(), x.grad.detach()


def loss_eval(head, pred, target, normalize=True):
    """(loss, d loss / d pred) in the dtype of the head's weights."""
    dt = next(head.parameters()).dtype
    p = pred.detach().to(dt).requires_grad_(True)
    t = target.detach().to(dt)
    a, b = (vnorm(p), vnorm(t)) if normalize else (p, t)
    loss = nn.functional.mse_loss(head(a), head(b))
    loss.backward()
    return loss.detach(), p.grad.detach()


def max_err(got, ref):
    """(max |got - ref|, max |ref|) in float64."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max()), float(ref.abs().max())


def bar(contract, err32, scale):
    """The bound on max |device - fp64|: the contract, or twice what torch's fp32 CPU evaluation misses fp64 by."""
    return max(contract * scale, 2.0 * err32)


@functools.lru_cache(maxsize=None)
def head_case(feature_layer, shape):
    """Inputs and fp64 / fp32-CPU results of one head case, computed once: dict with x, g, f64, dx64, f_err32, dx_err32."""
    h32, h64, _ = filled_head(feature_layer)
    x = fill.rand(shape, 700 + feature_layer + shape[2])
    f64, _ = head_eval(h64, x, torch.zeros(1))
    g = fill.randn(tuple(f64.shape), 710 + feature_layer + shape[2])
    f64, dx64 = head_eval(h64, x, g)
    f32, dx32 = head_eval(h32, x, g)
    return {"x": x, "g": g, "f64": f64, "dx64": dx64, "f_err32": max_err(f32, f64)[0], "dx_err32": max_err(dx32, dx64)[0]}


@functools.lru_cache(maxsize=None)
def loss_case(shape):
    h32, h64, _ = filled_head(8)
    pred, target = fill.rand(shape, 720 + shape[2]), fill.rand(shape, 730 + shape[2])
    l64, d64 = loss_eval(h64, pred, target)
    l32, d32 = loss_eval(h32, pred, target)
    return {"pred": pred, "target": target, "l64": float(l64), "d64": d64, "l_err32": abs(float(l32) - float(l64)),
            "d_err32": max_err(d32, d64)[0]}


# -- pool inputs ------------------------------------------------------------------------------------------------------
POOL_KINDS = ("continuous", "ties", "relu")


def pool_input(shape, kind, seed=740):
    if kind == "continuous":
        return fill.randn(shape, seed)
    if kind == "ties":      # values in {0, 1, 2}: about half of the windows hold their maximum more than once
        return torch.floor(fill.rand(shape, seed + 1, 0.0, 3.0)).clamp_(0, 2)
    # a ReLU output with whole windows of zeros: a coarse mask zeroes 2x2-aligned blocks, the rest is relu(randn)
    n, c, h, w = shape
    keep = (fill.rand((n, c, (h + 1) // 2, (w + 1) // 2), seed + 2) > 0.4).float()
    keep = keep.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w]
    return torch.relu(fill.randn(shape, seed + 3)) * keep


def pool_grad_cpu(x, dy):
    """ATen's CPU max_pool2d autograd, x and dy in the memory formats they arrive in."""
    xr = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    nn.functional.max_pool2d(xr, 2, 2).backward(dy)
    return xr.grad.detach()


# -- the child process of the data-parallel step test ----------------------------------------------------------------
def _dp_child():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      SRK_DP_FORCE_COMM="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    G, D = pkg.SRGANGenerator(3, 16, 2), pkg.SRGANDiscriminator(3, 8, 32)
    fill.fill_module(G, 5, 0.7)
    fill.fill_module(D, 6, 1.0)
    G.to(dev).train()
    D.to(dev).train()
    gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt, d_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-3), pkg.optim.make_optimizer("srgan_d", dflat, 1e-2)
    g_dp, d_dp = pkg.dp.DataParallel(gflat), pkg.dp.DataParallel(dflat)
    assert g_dp.active and d_dp.active
    fe = pkg.FeatureExtractor().load_vgg19(filled_head(8, 78)[2]).to(dev)
    before = gflat.data.clone()
    step = pkg.trainers.srgan_step(G, D, g_opt, d_opt, g_dp, d_dp, feature_extractor=fe, perceptual=True)
    d_loss, g_loss = step(fill.rand((2, 3, 8, 8), 670).to(dev), fill.rand((2, 3, 32, 32), 671).to(dev))
    d_loss, g_loss = d_loss.detach(), g_loss.detach()
    torch.cuda.synchronize()
    ok = bool(np.isfinite(float(d_loss)) and np.isfinite(float(g_loss)) and not torch.equal(before, gflat.data)
              and all(p.grad is None for p in fe.parameters()))
    print("dp-child d_loss %.8f g_loss %.8f ok %d" % (float(d_loss), float(g_loss), ok))
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:] == ["dp-child"]:
        sys.exit(_dp_child())
    sys.exit("usage: perceptual_ref.py dp-child")
