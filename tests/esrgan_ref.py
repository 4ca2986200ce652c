"""The fp64 restatement of ESRGAN's parts: the slice convolution with a scaled output and two scaled skips, the
residual-in-residual dense block with torch.cat, RRDBNet with BasicSR's parameter names, and the relativistic average
GAN loss through autograd.  Everything the ESRGAN tests compare against comes from here; nothing in it touches the
package's kernels.  Buffers and the single-convolution helpers are those of tests/rdn_ref.py."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import rdn_ref as R

SLOPE = 0.2
RES_SCALE = 0.2


# ---- the relativistic average GAN loss -----------------------------------------------------------------------------------
def ragan(real, fake, for_generator):
    """real, fake: [B] double tensors (leaves or not).  The mean over both rows of softplus, the means NOT detached."""
    a = real - fake.mean()
    b = fake - real.mean()
    if for_generator:
        return 0.5 * (F.softplus(a).mean() + F.softplus(-b).mean())
    return 0.5 * (F.softplus(-a).mean() + F.softplus(b).mean())


def ragan_grads(real, fake, for_generator):
    """(loss, d_real, d_fake) in double through autograd."""
    r = real.double().reshape(-1).clone().requires_grad_(True)
    f = fake.double().reshape(-1).clone().requires_grad_(True)
    loss = ragan(r, f, for_generator)
    loss.backward()
    return loss.detach(), r.grad, f.grad


def _logits(b, seed, std=2.0):
    rs = np.random.RandomState(seed)
    return (torch.from_numpy((std * rs.standard_normal(b)).astype(np.float32)),
            torch.from_numpy((std * rs.standard_normal(b) - 0.5).astype(np.float32)))


def _extreme(b, seed):
    r, f = _logits(b, seed)
    r[0], f[0] = 60.0, -60.0
    if b > 1:
        r[1], f[1] = -60.0, 60.0
    return r, f


def _equal(b, seed):
    r, _ = _logits(b, seed)
    return r, r.clone()


# name -> (real, fake): every B of the issue in its plain form, the +-60 logits, real == fake
RAGAN_CASES = {}
for _b in (1, 2, 3, 16, 257):
    RAGAN_CASES["B%d" % _b] = _logits(_b, 100 + _b)
    RAGAN_CASES["B%d_extreme" % _b] = _extreme(_b, 200 + _b)
RAGAN_CASES["B16_equal"] = _equal(16, 316)
RAGAN_CASES["B3_equal"] = _equal(3, 303)


# ---- the slice convolution with the RRDB epilogue ---------------------------------------------------------------------------
# (s, r1, R1 present, r2, R2 present, a1): the plain operator, each scale alone, and the two conv5 forms of an RRDB
EPILOGUES = {
    "plain": (1.0, 1.0, True, 0.0, False, 1.0),
    "s_only": (0.2, 1.0, False, 0.0, False, 1.0),
    "rdb": (0.2, 1.0, True, 0.0, False, 1.0),
    "r2_only": (1.0, 1.0, False, 0.5, True, 0.25),
    "rrdb": (0.04, 0.2, True, 1.0, True, 0.2),
    "all_odd": (-1.5, 0.75, True, -0.3, True, -2.0),
}


def conv_ex_forward(a, b, w, bias, act, s, r1, R1, r2, R2):
    y = s * R.conv_forward(a, b, w, bias, act, SLOPE)
    if R1 is not None:
        y = y + r1 * R1.double()
    if R2 is not None:
        y = y + r2 * R2.double()
    return y


def conv_ex_grads(a, b, w, bias, dy, act, s):
    """(da, db, dw, dbias) of sum(s * act(conv) * dy): g = s * dy * act'."""
    _, da, db, dw, dbias = R.conv_grads(a, b, w, bias, dy.double() * s, act, SLOPE)
    return da, db, dw, dbias


# ---- the block, the trunk, the net -------------------------------------------------------------------------------------------
def dense5_forward(x, p, rs):
    """One dense block: p = (w1, b1, ..., w5, b5), in whatever dtype x and p have."""
    feats = x
    for c in range(4):
        feats = torch.cat((feats, F.leaky_relu(F.conv2d(feats, p[2 * c], p[2 * c + 1], padding=1), SLOPE)), 1)
    return rs * F.conv2d(feats, p[8], p[9], padding=1) + x


def rrdb_forward(x, rrdb, rs=RES_SCALE):
    out = x
    for p in rrdb:
        out = dense5_forward(out, p, rs)
    return rs * out + x


def trunk_forward(x, blocks, rs=RES_SCALE):
    for b in blocks:
        x = rrdb_forward(x, b, rs)
    return x


def make_blocks(f, g, nb, seed, gain=1.0):
    blocks = []
    for i in range(nb):
        rrdb = []
        for k in range(3):
            p = []
            for c in range(5):
                cin, cout = f + c * g, (g if c < 4 else f)
                s0 = seed + 1000 * i + 100 * k + 2 * c
                p.append(R.rand((cout, cin, 3, 3), s0, gain * (2.0 / (cin * 9)) ** 0.5))
                p.append(R.rand((cout,), s0 + 1, 0.05))
            rrdb.append(tuple(p))
        blocks.append(tuple(rrdb))
    return blocks


def to64(blocks, requires_grad=False):
    return [tuple(tuple(t.detach().cpu().double().requires_grad_(requires_grad) for t in p) for p in b) for b in blocks]


class _RefDense5(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        for c in range(4):
            setattr(self, "conv%d" % (c + 1), nn.Conv2d(nf + c * gc, gc, 3, padding=1))
        self.conv5 = nn.Conv2d(nf + 4 * gc, nf, 3, padding=1)

    def forward(self, x):
        feats = x
        for c in range(4):
            feats = torch.cat((feats, F.leaky_relu(getattr(self, "conv%d" % (c + 1))(feats), SLOPE)), 1)
        return RES_SCALE * self.conv5(feats) + x


class _RefRRDB(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _RefDense5(nf, gc), _RefDense5(nf, gc), _RefDense5(nf, gc)

    def forward(self, x):
        return RES_SCALE * self.rdb3(self.rdb2(self.rdb1(x))) + x


class RefRRDBNet(nn.Module):
    """RRDBNet (x4) in plain torch with BasicSR's parameter names; loads the package's state_dict."""

    def __init__(self, num_channels, nf=64, nb=23, gc=32):
        super().__init__()
        self.conv_first = nn.Conv2d(num_channels, nf, 3, padding=1)
        self.body = nn.ModuleList([_RefRRDB(nf, gc) for _ in range(nb)])
        self.conv_body = nn.Conv2d(nf, nf, 3, padding=1)
        self.conv_up1 = nn.Conv2d(nf, nf, 3, padding=1)
        self.conv_up2 = nn.Conv2d(nf, nf, 3, padding=1)
        self.conv_hr = nn.Conv2d(nf, nf, 3, padding=1)
        self.conv_last = nn.Conv2d(nf, num_channels, 3, padding=1)

    def forward(self, x):
        feat = self.conv_first(x)
        out = feat
        for b in self.body:
            out = b(out)
        out = self.conv_body(out) + feat
        out = F.leaky_relu(self.conv_up1(F.interpolate(out, scale_factor=2, mode="nearest")), SLOPE)
        out = F.leaky_relu(self.conv_up2(F.interpolate(out, scale_factor=2, mode="nearest")), SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(out), SLOPE))


def ref_net_like(net, *ctor):
    ref = RefRRDBNet(*ctor).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref


def state_table(num_channels, nf, nb, gc):
    """name -> shape of RRDBNet's state_dict, written out from the architecture."""
    t = {}

    def conv(name, cin, cout):
        t[name + ".weight"], t[name + ".bias"] = (cout, cin, 3, 3), (cout,)

    conv("conv_first", num_channels, nf)
    for i in range(nb):
        for k in (1, 2, 3):
            for c in range(5):
                conv("body.%d.rdb%d.conv%d" % (i, k, c + 1), nf + c * gc, gc if c < 4 else nf)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, nf, nf)
    conv("conv_last", nf, num_channels)
    return t


# ---- the full step, in fp32 on the CPU ----------------------------------------------------------------------------------------
def ref_discriminator(num_channels, base_filter, image_size):
    """The oracle's SRGAN discriminator ending in a logit (what models.ESRGANDiscriminator is)."""
    from oracle import ref_modules as M
    d = M.Discriminator(num_channels, base_filter, image_size)
    d.dense_layers[1] = M.DenseBlock(base_filter * 16, 1, activation=None, norm=None)
    return d


def oracle_pretrain_step(G, g_opt, lr_img, hr_img):
    g_opt.zero_grad()
    loss = F.l1_loss(G(lr_img), hr_img)
    loss.backward()
    g_opt.step()
    return float(loss.detach())


def oracle_adversarial_step(G, D, g_opt, d_opt, head, vnorm, lr_img, hr_img, pixel_w=1e-2, vgg_w=1.0, gan_w=5e-3):
    """trainers.esrgan_segments restated with stock torch: the G step with D frozen, then the D step; D in training mode
    in all four of its forwards (its BatchNorm statistics move in each).  Returns (d_loss, g_loss)."""
    for p in D.parameters():
        p.requires_grad_(False)
    g_opt.zero_grad()
    fake = G(lr_img)
    real_logits = D(hr_img).detach()
    l_gan = ragan(real_logits.reshape(-1), D(fake).reshape(-1), True)
    l_pix = F.l1_loss(fake, hr_img)
    l_vgg = F.l1_loss(head(vnorm(fake)), head(vnorm(hr_img)).detach())
    g_loss = pixel_w * l_pix + vgg_w * l_vgg + gan_w * l_gan
    g_loss.backward()
    g_opt.step()
    for p in D.parameters():
        p.requires_grad_(True)
    d_opt.zero_grad()
    d_loss = ragan(D(hr_img).reshape(-1), D(fake.detach()).reshape(-1), False)
    d_loss.backward()
    d_opt.step()
    return float(d_loss.detach()), float(g_loss.detach())
