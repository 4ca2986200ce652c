"""The torch restatement of Real-ESRGAN's U-Net discriminator and of its three operators, written from the published
architecture (Wang et al., "Real-ESRGAN", ICCVW 2021): torch.nn.utils.spectral_norm (the legacy hook form), F.interpolate
(bilinear, align_corners=False) and softplus, all on the CPU.  Everything the Real-ESRGAN tests compare against comes from
here; nothing in it touches the package's kernels."""
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import spectral_norm

SLOPE = 0.2
EPS = 1e-12

# the filter shapes of the issue: [out, in, kh, kw]
SN_SHAPES = [(1, 1, 1, 1), (1, 7, 1, 1), (5, 1, 1, 1), (3, 3, 3, 3), (16, 3, 4, 4), (64, 64, 3, 3), (130, 13, 3, 3),
             (128, 64, 4, 4), (512, 256, 4, 4)]
# (N, H, W, C)
BILINEAR_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (1, 4, 1, 2), (2, 2, 2, 1), (2, 3, 5, 7), (1, 8, 8, 64), (2, 5, 9, 130)]
GAN_SIZES = [1, 3, 255, 256, 257, 4097, 65536]


def _rs(seed, name=""):
    return np.random.RandomState((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 31))


def randn(shape, seed, std=1.0):
    return torch.from_numpy((_rs(seed).standard_normal(shape) * std).astype(np.float32))


def worst(got, want):
    """max |got - want| over max |want|, in double on the CPU."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---- spectral normalisation ---------------------------------------------------------------------------------------------
def sn_case(shape, seed):
    """(W, u, v) fp32: a filter at He scale and normalised standard normals, as torch initialises them."""
    r, k = shape[0], int(np.prod(shape[1:]))
    w = randn(shape, seed, (2.0 / k) ** 0.5)
    u, v = randn((r,), seed + 1), randn((k,), seed + 2)
    return w, u / u.norm().clamp_min(EPS), v / v.norm().clamp_min(EPS)


class _OneConv(nn.Module):
    def __init__(self, w, u, v, dtype):
        super().__init__()
        o, i, kh, kw = w.shape
        conv = nn.Conv2d(i, o, (kh, kw), bias=False).to(dtype)
        self.conv = spectral_norm(conv, n_power_iterations=1, eps=EPS, dim=0)
        with torch.no_grad():
            self.conv.weight_orig.copy_(w.to(dtype))
            self.conv.weight_u.copy_(u.to(dtype))
            self.conv.weight_v.copy_(v.to(dtype))

    def weight(self):
        """Runs the hook once (training mode: one power iteration, in place) and returns the normalised filter, attached."""
        o, i, kh, kw = self.conv.weight_orig.shape
        self.conv(torch.zeros(1, i, kh, kw, dtype=self.conv.weight_orig.dtype))
        return self.conv.weight


def sn_module(w, u, v, dtype=torch.float64):
    return _OneConv(w, u, v, dtype)


def sn_reference(w, u, v, training, g=None, dtype=torch.float64):
    """One forward of torch's spectral_norm on (w, u, v) -> dict(w_sn, u, v, sigma, dW): u and v after the call, dW the
    gradient of sum(w_sn * g) where g is given."""
    m = sn_module(w, u, v, dtype)
    m.train(training)
    w_sn = m.weight()
    out = {"w_sn": w_sn.detach().clone(), "u": m.conv.weight_u.detach().clone(), "v": m.conv.weight_v.detach().clone()}
    wm = m.conv.weight_orig.detach().reshape(w.shape[0], -1)
    out["sigma"] = float(torch.dot(out["u"], wm @ out["v"]))
    if g is not None:
        (w_sn * g.to(dtype)).sum().backward()
        out["dW"] = m.conv.weight_orig.grad.detach().clone()
    return out


# ---- bilinear x2 ------------------------------------------------------------------------------------------------------------
def bilinear_reference(x_nhwc, add_nhwc=None, dy_nhwc=None):
    """(y, dx) in double, NHWC in and out; dx = the gradient of sum(y * dy) (None without dy)."""
    x = x_nhwc.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    s = x if add_nhwc is None else x + add_nhwc.double().permute(0, 3, 1, 2)
    y = F.interpolate(s, scale_factor=2, mode="bilinear", align_corners=False)
    dx = None
    if dy_nhwc is not None:
        (y * dy_nhwc.double().permute(0, 3, 1, 2)).sum().backward()
        dx = x.grad.permute(0, 2, 3, 1).contiguous()
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx


# ---- the vanilla GAN loss on logits --------------------------------------------------------------------------------------------
def gan_logits(n, seed, extreme=False):
    x = randn((n,), seed, 2.0)
    if extreme:
        x[0] = 60.0
        x[-1] = -60.0
    return x


def gan_reference(x, target_is_real):
    """(loss, dx) in double: mean softplus(-x) for a real target, mean softplus(x) for a fake one."""
    x = x.double().clone().requires_grad_(True)
    loss = F.softplus(-x).mean() if target_is_real else F.softplus(x).mean()
    loss.backward()
    return loss.detach(), x.grad


def gan_loss(logits, target_is_real):
    """The same through BCE-with-logits, the form BasicSR's GANLoss('vanilla') computes."""
    t = torch.ones_like(logits) if target_is_real else torch.zeros_like(logits)
    return F.binary_cross_entropy_with_logits(logits, t)


# ---- the net ------------------------------------------------------------------------------------------------------------------
class RefUNetDiscriminatorSN(nn.Module):
    """The U-Net discriminator with spectral normalisation in stock torch, under the published parameter names."""

    def __init__(self, num_in_ch=3, num_feat=64, skip_connection=True):
        super().__init__()
        f, sn = num_feat, spectral_norm
        self.skip_connection = skip_connection
        self.conv0 = nn.Conv2d(num_in_ch, f, 3, 1, 1)
        self.conv1 = sn(nn.Conv2d(f, 2 * f, 4, 2, 1, bias=False))
        self.conv2 = sn(nn.Conv2d(2 * f, 4 * f, 4, 2, 1, bias=False))
        self.conv3 = sn(nn.Conv2d(4 * f, 8 * f, 4, 2, 1, bias=False))
        self.conv4 = sn(nn.Conv2d(8 * f, 4 * f, 3, 1, 1, bias=False))
        self.conv5 = sn(nn.Conv2d(4 * f, 2 * f, 3, 1, 1, bias=False))
        self.conv6 = sn(nn.Conv2d(2 * f, f, 3, 1, 1, bias=False))
        self.conv7 = sn(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv8 = sn(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(f, 1, 3, 1, 1)

    def forward(self, x):
        act = lambda t: F.leaky_relu(t, SLOPE)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
        x0 = act(self.conv0(x))
        x1 = act(self.conv1(x0))
        x2 = act(self.conv2(x1))
        x3 = act(self.conv3(x2))
        x4 = act(self.conv4(up(x3)))
        if self.skip_connection:
            x4 = x4 + x2
        x5 = act(self.conv5(up(x4)))
        if self.skip_connection:
            x5 = x5 + x1
        x6 = act(self.conv6(up(x5)))
        if self.skip_connection:
            x6 = x6 + x0
        out = act(self.conv7(x6))
        out = act(self.conv8(out))
        return self.conv9(out)


def fill_discriminator(net, seed):
    """Deterministic state for either net (the same keys): filters at He scale, biases 0.05 N, u and v normalised normals."""
    sd = net.state_dict()
    with torch.no_grad():
        for name in sorted(sd):
            t, rs = sd[name], _rs(seed, name)
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("weight", "weight_orig") and t.dim() == 4:
                val = rs.standard_normal(tuple(t.shape)) * np.sqrt(2.0 / int(np.prod(t.shape[1:])))
            elif leaf in ("weight_u", "weight_v"):
                val = rs.standard_normal(tuple(t.shape))
                val = val / max(np.sqrt((val * val).sum()), EPS)
            elif leaf == "bias":
                val = 0.05 * rs.standard_normal(tuple(t.shape))
            else:
                continue          # (`weight` of the hook form: recomputed by every forward)
            t.copy_(torch.from_numpy(np.asarray(val, dtype=np.float32)).to(t.dtype))
    return net


def ref_like(net, num_in_ch, num_feat, dtype=torch.float64, skip_connection=True):
    """The restatement holding `net`'s state (a package UNetDiscriminatorSN, on any device)."""
    ref = RefUNetDiscriminatorSN(num_in_ch, num_feat, skip_connection).to(dtype)
    missing = ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return ref


def state_table(num_in_ch, f):
    """name -> shape of the discriminator's state_dict, written out from the architecture."""
    t = {"conv0.weight": (f, num_in_ch, 3, 3), "conv0.bias": (f,)}
    for name, cin, cout, k in (("conv1", f, 2 * f, 4), ("conv2", 2 * f, 4 * f, 4), ("conv3", 4 * f, 8 * f, 4),
                               ("conv4", 8 * f, 4 * f, 3), ("conv5", 4 * f, 2 * f, 3), ("conv6", 2 * f, f, 3),
                               ("conv7", f, f, 3), ("conv8", f, f, 3)):
        t[name + ".weight_orig"], t[name + ".weight_u"], t[name + ".weight_v"] = (cout, cin, k, k), (cout,), (cin * k * k,)
    t["conv9.weight"], t["conv9.bias"] = (1, f, 3, 3), (1,)
    return t


# ---- the full step, in fp32 on the CPU -----------------------------------------------------------------------------------------
def oracle_vanilla_step(G, D, g_opt, d_opt, head, vnorm, lr_img, hr_img, pixel_w=1e-2, vgg_w=1.0, gan_w=5e-3):
    """trainers.esrgan_segments(gan_type='vanilla') restated with stock torch, BasicSR's SRGAN order: the G step with D
    frozen (one D forward), then the D step (two): D runs three training-mode forwards.  Returns (d_loss, g_loss)."""
    for p in D.parameters():
        p.requires_grad_(False)
    g_opt.zero_grad()
    fake = G(lr_img)
    l_gan = gan_loss(D(fake), True)
    l_pix = F.l1_loss(fake, hr_img)
    l_vgg = F.l1_loss(head(vnorm(fake)), head(vnorm(hr_img)).detach())
    g_loss = pixel_w * l_pix + vgg_w * l_vgg + gan_w * l_gan
    g_loss.backward()
    g_opt.step()
    for p in D.parameters():
        p.requires_grad_(True)
    d_opt.zero_grad()
    d_loss = gan_loss(D(hr_img), True) + gan_loss(D(fake.detach()), False)
    d_loss.backward()
    d_opt.step()
    return float(d_loss.detach()), float(g_loss.detach())
