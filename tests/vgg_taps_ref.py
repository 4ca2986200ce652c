"""The yardstick of the multi-layer VGG feature loss tests (ops.vgg_feature_loss, csrc/vgg_tap.hip): one tapped layer and
the whole term restated with stock torch layers -- relu, max_pool2d, l1_loss and autograd on the CPU, in float64 -- the
case tables of tests/test_vgg_taps_cpu.py and tests/test_vgg_taps_gpu.py, the same term composed from the operators the
package had before the fused tap, and the fp32 CPU oracle of an ESRGAN step that trains on the term.

Bars.  One tap: the pooled and ReLU maps are selections of fp32 inputs, so they are bit-equal to torch; the loss is held
to the project's 1e-4 relative contract (the sum is fp64 on both sides: about 1e-7 is expected, the fp32 store of the
result); da to 1e-3 * max|ref| (expected: one fp32 rounding).  The host twins are fp64 up to their fp32 stores: loss
within 1e-12 relative (summation order), da within fp32 rounding of the fp64 value.  The whole term goes through a chain
of fp32 convs whose ReLU, pool and sign decisions can flip within rounding: perceptual_ref.bar, the contract or twice
torch's own fp32 CPU error on the same inputs."""
import ctypes
import functools

import torch
import torch.nn.functional as F

import esrgan_ref as E
import perceptual_ref as P
from oracle import fill

POOL, RELU, LAST = 0, 1, 2     # srk_vgg_tap_mode
MODES = {"pool": POOL, "relu": RELU, "last": LAST}
REALESRGAN = (("conv1_2", 0.1), ("conv2_2", 0.1), ("conv3_4", 1.0), ("conv4_4", 1.0), ("conv5_4", 1.0))
REALESRGAN_INDEX = {"conv1_2": 2, "conv2_2": 7, "conv3_4": 16, "conv4_4": 25, "conv5_4": 34}
LOSS_CONTRACT, GRAD_CONTRACT, HOST_LOSS_TOL = 1e-4, 1e-3, 1e-12
FP32_EPS = 2.0 ** -24          # half an ulp of 1: the rounding of one fp32 store, relative

# (N, C, H, W): scalar and 16-byte paths, odd trailing rows and columns, one-window planes, several blocks
OP_SHAPES = [(1, 1, 2, 2), (1, 3, 2, 3), (1, 4, 3, 2), (1, 5, 7, 9), (2, 8, 6, 10), (1, 64, 2, 2), (2, 64, 34, 38)]
LAST_ONLY_SHAPES = [(1, 512, 1, 1)]
KINDS = ("continuous", "ties", "nonpositive")
TERM_SHAPES = [(2, 3, 16, 16), (1, 3, 20, 18)]


def op_cases():
    """[(shape, mode name)]: every shape in every mode, the 1 x 1 plane in LAST alone."""
    return [(s, m) for s in OP_SHAPES for m in MODES] + [(s, "last") for s in LAST_ONLY_SHAPES]


def conv_names(cfg=P.VGG19_CFG):
    """{'conv{k}_{j}': torchvision index} from the stock configuration tuple."""
    names, idx, k, j = {}, 0, 1, 0
    for v in cfg:
        if v == 'M':
            idx, k, j = idx + 1, k + 1, 0
        else:
            j += 1
            names["conv%d_%d" % (k, j)] = idx
            idx += 2
    return names


def tap_inputs(shape, kind, seed=900):
    """(a, b): fp32 NCHW maps of one layer before its ReLU."""
    seed += shape[1] * 7 + shape[2] * 3 + shape[3]
    if kind == "continuous":
        return fill.randn(shape, seed), fill.randn(shape, seed + 1)
    if kind == "ties":     # a small grid {-1, 0, 1, 2}: a == b occurs, and equal positive values share a window
        return torch.floor(fill.rand(shape, seed + 2, -1.0, 3.0)), torch.floor(fill.rand(shape, seed + 3, -1.0, 3.0))
    # whole 2 x 2-aligned windows without a positive value (exact zeros among them); the rest continuous
    n, c, h, w = shape
    a, b = fill.randn(shape, seed + 4), fill.randn(shape, seed + 5)
    dead = (fill.rand((n, c, (h + 1) // 2, (w + 1) // 2), seed + 6) > 0.5).float()
    dead = dead.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w]
    zero = (fill.rand(shape, seed + 7) > 0.7).float()
    a = a * (1 - dead) + (-a.abs() * (1 - zero)) * dead
    return a, b


def behind(x, mode):
    """What the head runs behind the tap, stock torch in the dtype of x (None at the end of the walk)."""
    if mode == POOL:
        return F.max_pool2d(torch.relu(x), 2, 2)
    return torch.relu(x) if mode == RELU else None


def out_shape(shape, mode):
    n, c, h, w = shape
    return (n, c, h // 2, w // 2) if mode == POOL else (n, c, h, w)


@functools.lru_cache(maxsize=None)
def tap_case(shape, mode_name, kind, weight=0.7, seed_value=1.0):
    """One operator case, computed once: a, b, g (the gradient of the map behind the tap), and from float64 autograd the
    loss and da = d(seed * loss + sum(ya * g)) / da; ya, yb from the same stock layers in fp32."""
    mode = MODES[mode_name]
    a, b = tap_inputs(shape, kind)
    g = fill.randn(out_shape(shape, mode), 950 + shape[2]) if mode != LAST else None
    a64 = a.double().requires_grad_(True)
    loss = weight * F.l1_loss(a64, b.double())
    total = seed_value * loss
    if mode != LAST:
        total = total + (behind(a64, mode) * g.double()).sum()
    total.backward()
    return {"a": a, "b": b, "g": g, "mode": mode, "weight": weight, "seed": seed_value, "loss": float(loss.detach()),
            "da": a64.grad.detach(), "ya": behind(a, mode), "yb": behind(b, mode),
            "c": weight * seed_value / a.numel()}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host_forward(lib, a, b, mode, weight):
    """srk_vgg_tap_forward_host on NCHW CPU tensors -> (loss, ya, yb), the maps NCHW views pre-filled with NaN."""
    n, c, h, w = a.shape
    an, bn = nhwc(a), nhwc(b)
    ya = yb = None
    if mode != LAST:
        on, oc, oh, ow = out_shape(a.shape, mode)
        ya, yb = torch.full((on, oh, ow, oc), float("nan")), torch.full((on, oh, ow, oc), float("nan"))
    loss = ctypes.c_double(float("nan"))
    rc = lib.srk_vgg_tap_forward_host(_p(an), _p(bn), n, h, w, c, mode, weight, ctypes.byref(loss), _p(ya), _p(yb))
    assert rc == 0, lib.srk_last_error_string()
    return loss.value, None if ya is None else nchw(ya), None if yb is None else nchw(yb)


def host_backward(lib, a, b, g, mode, c_value):
    n, c, h, w = a.shape
    an, bn, gn = nhwc(a), nhwc(b), None if g is None else nhwc(g)
    da = torch.full((n, h, w, c), float("nan"))
    rc = lib.srk_vgg_tap_backward_host(_p(an), _p(bn), _p(gn), n, h, w, c, mode, c_value, _p(da))
    assert rc == 0, lib.srk_last_error_string()
    return nchw(da)


def plan_of(lib, shape, mode, vec):
    """(blocks, items, passes of a block's grid-stride loop) of the launcher's own plan."""
    n, c, h, w = shape
    items = ctypes.c_longlong(0)
    blocks = lib.srk_vgg_tap_plan(n, h, w, c, mode, vec, ctypes.byref(items))
    assert blocks > 0, lib.srk_last_error_string()
    return blocks, items.value, -(-items.value // (blocks * 256))


def multi_chunk_shape(lib, mode=POOL):
    """The smallest even square plane of 64 channels at which a block of the 16-byte path walks more than one chunk,
    found by asking the launcher's plan."""
    side = 2
    while plan_of(lib, (1, 64, side, side), mode, 1)[2] < 2:
        side += 2
        assert side <= 4096
    return (1, 64, side, side)


# ---- the whole term ----------------------------------------------------------------------------------------------------
def head_taps(head, x, indices):
    """{index: the map that leaves module `index`} of a stock head (its ReLUs are not in place)."""
    got = {}
    for i, m in enumerate(head):
        x = m(x)
        if i in indices:
            got[i] = x
        if i >= max(indices):
            break
    return got


def term(head, pred, target, layers=REALESRGAN, normalize=True):
    """sum_k w_k * L1 of the maps before the ReLUs, in the dtype of the operands; the target's maps carry no graph."""
    index = conv_names()
    want = [(index[name], w) for name, w in layers if w > 0]
    a, b = (P.vnorm(pred), P.vnorm(target)) if normalize else (pred, target)
    fa = head_taps(head, a, [i for i, _ in want])
    with torch.no_grad():
        fb = head_taps(head, b, [i for i, _ in want])
    return sum(w * F.l1_loss(fa[i], fb[i]) for i, w in want)


def term_eval(head, pred, target, layers=REALESRGAN, normalize=True):
    """(loss, d loss / d pred) in the dtype of the head's weights."""
    dt = next(head.parameters()).dtype
    p = pred.detach().to(dt).requires_grad_(True)
    loss = term(head, p, target.detach().to(dt), layers, normalize)
    loss.backward()
    return float(loss.detach()), p.grad.detach()


@functools.lru_cache(maxsize=None)
def term_case(shape, vgg_seed=77):
    h32, h64, sd = P.filled_head(34, vgg_seed)
    pred, target = fill.rand(shape, 820 + shape[2]), fill.rand(shape, 830 + shape[2])
    l64, d64 = term_eval(h64, pred, target)
    l32, d32 = term_eval(h32, pred, target)
    return {"pred": pred, "target": target, "l64": l64, "d64": d64, "l_err32": abs(l32 - l64),
            "d_err32": P.max_err(d32, d64)[0], "sd": sd}


def composition(pkg, extractor, pred, target, layers=REALESRGAN, normalize=True):
    """The same term from the operators the package had before the fused tap: every tapped conv un-fused, the tapped map
    forked (ops.fork), ops.l1_loss on the pair, then a ReLU launch (ops.activation) and ops.max_pool2x2_train; the terms
    added by ops.loss_sum.  Both operands on the same kernels, the target's without a graph."""
    ops = pkg.ops
    act_relu, act_none = pkg._lib.ACT_RELU, pkg._lib.ACT_NONE
    index = conv_names()
    want = dict((index[name], w) for name, w in layers if w > 0)
    last = max(want)
    a = pkg.utils.norm(pred, vgg=True) if normalize else pred
    with torch.no_grad():
        b = pkg.utils.norm(target.detach(), vgg=True) if normalize else target.detach()
    mods = list(extractor.features)
    terms, i = [], 0
    while i <= last:
        m = mods[i]
        if isinstance(m, torch.nn.Conv2d):
            fused = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
            tapped = i in want
            cfg = ops.ConvCfg(m._s, m._p, False, 0, act_relu if (fused and not tapped) else act_none)
            packs = m._cache.get(m.weight, m.bias, False, 0, bwd=True)
            a = ops.conv2d(a, m.weight, m.bias, None, cfg, packs)
            with torch.no_grad():
                b = ops.conv2d(b, m.weight, m.bias, None, cfg, packs)
            if tapped:
                if i < last:
                    keep, a = ops.fork(a)
                else:
                    keep = a
                terms.append((ops.l1_loss(keep, b), want[i]))
                if i < last and fused:
                    a = ops.activation(a, act_relu)
                    with torch.no_grad():
                        b = ops.activation(b, act_relu)
            i += 2 if fused else 1
        else:
            a = ops.max_pool2x2_train(a)
            with torch.no_grad():
                b = ops.max_pool2x2_train(b)
            i += 1
    (t0, w0) = terms[0]
    if len(terms) == 1:
        return ops.loss_sum(t0, t0, w0, 0.0)
    total = ops.loss_sum(t0, terms[1][0], w0, terms[1][1])
    for t, w in terms[2:]:
        total = ops.loss_sum(total, t, 1.0, w)
    return total


# ---- the ESRGAN step that trains on the term, in fp32 on the CPU ------------------------------------------------------------
def oracle_adversarial_step(G, D, g_opt, d_opt, head, lr_img, hr_img, layers=REALESRGAN, pixel_w=1e-2, vgg_w=1.0, gan_w=5e-3):
    """esrgan_ref.oracle_adversarial_step with the multi-layer term in the place of its single conv5_4 one."""
    for p in D.parameters():
        p.requires_grad_(False)
    g_opt.zero_grad()
    fake = G(lr_img)
    real_logits = D(hr_img).detach()
    l_gan = E.ragan(real_logits.reshape(-1), D(fake).reshape(-1), True)
    l_pix = F.l1_loss(fake, hr_img)
    l_vgg = term(head, fake, hr_img, layers)
    g_loss = pixel_w * l_pix + vgg_w * l_vgg + gan_w * l_gan
    g_loss.backward()
    g_opt.step()
    for p in D.parameters():
        p.requires_grad_(True)
    d_opt.zero_grad()
    d_loss = E.ragan(D(hr_img).reshape(-1), D(fake.detach()).reshape(-1), False)
    d_loss.backward()
    d_opt.step()
    return float(d_loss.detach()), float(g_loss.detach())
