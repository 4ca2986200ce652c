"""Network topologies of the reference (srcnn.py:13-29, espcn.py:13-29, fsrcnn.py:13-55,
vdsr.py:13-36, edsr.py:13-45, lapsrn.py:14-85, srgan.py:14-81, drcn.py:13-59) built from the MI355X blocks.

Same constructor signatures, attribute names (=> state_dict keys), forward semantics and
`weight_init` distributions.  Differences are purely about launch count: residual adds are handed
to the producing conv's epilogue and tensors that fan out in training go through `ops.fork` so the
gradient fan-in is one srk_axpby launch.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, utils
from ._lib import ACT_NONE, ACT_RELU
from .base_networks import (RDB, RRDB, RSTB, ConvBlock, DeconvBlock, DenseBlock, PSBlock, ResidualGroup, ResnetBlock,
                            Upsample2xBlock)
from .layers import Conv2d, ConvTranspose2d, LayerNorm, LeakyReLU, PixelShuffle, PReLU, grad_mode
from ._lib import ACT_LRELU


def _training_graph(module, x):
    return grad_mode(x, *[p for p in module.parameters()])


class SRCNNNet(nn.Module):
    """srcnn.py:13-29 — 9-5-5, valid padding."""

    def __init__(self, num_channels, base_filter):
        super(SRCNNNet, self).__init__()
        self.layers = nn.Sequential(
            ConvBlock(num_channels, base_filter, 9, 1, 0, norm=None),
            ConvBlock(base_filter, base_filter // 2, 5, 1, 0, norm=None),
            ConvBlock(base_filter // 2, num_channels, 5, 1, 0, activation=None, norm=None))

    def forward(self, x):
        return self.layers(x)

    def weight_init(self, mean=0.0, std=0.001):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)


class ESPCNNet(nn.Module):
    """espcn.py:13-29 — 5-3-3 + PixelShuffle(r)."""

    def __init__(self, num_channels, base_filter, scale_factor):
        super(ESPCNNet, self).__init__()
        self.layers = nn.Sequential(
            ConvBlock(num_channels, base_filter, 5, 1, 0, activation='relu', norm=None),
            ConvBlock(base_filter, base_filter // 2, 3, 1, 0, activation='relu', norm=None),
            PSBlock(base_filter // 2, num_channels, scale_factor, 3, 1, 0, activation=None, norm=None))

    def forward(self, x):
        if ops.ESPCN_PAIR:
            y = ops.espcn_pair(x, self.layers[0], self.layers[1])
            if y is not None:
                return self.layers[2](y)
        return self.layers(x)

    def weight_init(self):
        for m in self.modules():
            utils.weights_init_normal(m)


class MotionCompensator(nn.Module):
    """The coarse-to-fine flow estimator of VESPCN (Caballero et al., CVPR 2017, table 1), for one pair of frames:
      coarse, on [cur | nbr] (2C channels): 5x5 s2 conv -> 24, 3x3 -> 24, 5x5 s2 -> 24, 3x3 -> 24 (ReLU each),
              3x3 -> 32 with tanh, PixelShuffle(4) -> 2 channels at the input size;
      fine, on [cur | nbr | coarse | flow_warp(nbr, max_flow * coarse)] (3C + 2): 5x5 s2 -> 24, three 3x3 -> 24 (ReLU
              each), 3x3 -> 8 with tanh, PixelShuffle(2).
    The flow in PIXELS is max_flow * coarse + max_flow / 4 * fine (x then y displacement); the paper states no scale,
    max_flow is this project's choice.  The fine stage sees the coarse flow in its tanh units.  H and W must be multiples
    of 4.  tanh is pointwise, so conv -> tanh -> shuffle is the PSBlock's conv -> shuffle -> tanh.  Key names: this
    project's own (coarse.{0..4}.conv, fine.{0..4}.conv); no upstream file exists."""

    def __init__(self, num_channels, max_flow=8.0):
        super(MotionCompensator, self).__init__()
        c = num_channels
        self.max_flow = float(max_flow)
        self.coarse = nn.Sequential(
            ConvBlock(2 * c, 24, 5, 2, 2, activation='relu', norm=None),
            ConvBlock(24, 24, 3, 1, 1, activation='relu', norm=None),
            ConvBlock(24, 24, 5, 2, 2, activation='relu', norm=None),
            ConvBlock(24, 24, 3, 1, 1, activation='relu', norm=None),
            PSBlock(24, 2, 4, 3, 1, 1, activation='tanh', norm=None))
        self.fine = nn.Sequential(
            ConvBlock(3 * c + 2, 24, 5, 2, 2, activation='relu', norm=None),
            ConvBlock(24, 24, 3, 1, 1, activation='relu', norm=None),
            ConvBlock(24, 24, 3, 1, 1, activation='relu', norm=None),
            ConvBlock(24, 24, 3, 1, 1, activation='relu', norm=None),
            PSBlock(24, 2, 2, 3, 1, 1, activation='tanh', norm=None))

    def forward(self, pair):
        """pair [M, 2C, H, W] = [cur | nbr] -> the flow [M, 2, H, W] in pixels that moves nbr onto cur."""
        c = pair.shape[1] // 2
        if pair.shape[2] % 4 or pair.shape[3] % 4:
            raise ValueError("MotionCompensator: a %d x %d input is not a multiple of 4 (two stride-2 stages)"
                             % (pair.shape[2], pair.shape[3]))
        coarse = self.coarse(pair)
        if _training_graph(self, pair):
            c_in, rest = ops.fork(coarse)     # three consumers: their gradients are added by srk_axpby
            c_warp, c_sum = ops.fork(rest)
        else:
            c_in = c_warp = c_sum = coarse
        warped = ops.flow_warp(pair[:, c:], ops.axpby(c_warp, None, self.max_flow))
        fine = self.fine(torch.cat([pair, c_in, warped], 1))
        return ops.axpby(c_sum, fine, self.max_flow, self.max_flow / 4.0)


class VESPCNNet(nn.Module):
    """VESPCN (Caballero et al., CVPR 2017), three frames, early fusion: the two neighbours are warped onto the centre
    frame by the MotionCompensator's flow (both through it as one batch of 2N) and [warp(t-1) | frame t | warp(t+1)] goes
    through ESPCN's 5-3-3 trunk (valid padding) with 3C input channels and PixelShuffle(r): the output is r (H - 8) on a
    side, to be held against the centre HR frame shaved by 4 r.
    x: [N,3,C,H,W] (t-1, t, t+1).  forward(x) -> sr; forward_terms(x) -> (sr, mc, flow): the motion-compensation loss
    of ops.motion_fuse and the flow [2N,2,H,W] in pixels, for the training loss.  Training refuses sides that are not
    multiples of 4; eval() replicate-pads the bottom and the right up to one and crops the result."""

    def __init__(self, num_channels, base_filter, scale_factor, max_flow=8.0):
        super(VESPCNNet, self).__init__()
        if not float(max_flow) > 0.0:
            raise ValueError("VESPCNNet: max_flow %r is not positive" % (max_flow,))
        self.num_channels, self.scale_factor = int(num_channels), int(scale_factor)
        self.mc = MotionCompensator(num_channels, max_flow)
        self.layers = nn.Sequential(
            ConvBlock(3 * num_channels, base_filter, 5, 1, 0, activation='relu', norm=None),
            ConvBlock(base_filter, base_filter // 2, 3, 1, 0, activation='relu', norm=None),
            PSBlock(base_filter // 2, num_channels, scale_factor, 3, 1, 0, activation=None, norm=None))

    def weight_init(self):
        for m in self.modules():
            utils.weights_init_normal(m)

    def check_image_size(self, x):
        if x.dim() != 5 or x.shape[1] != 3 or x.shape[2] != self.num_channels:
            raise ValueError("VESPCNNet: expects [N,3,%d,H,W] (frames t-1, t, t+1), got %s" % (self.num_channels, tuple(x.shape)))
        h, w = x.shape[3], x.shape[4]
        if min(h, w) < 9:
            raise ValueError("VESPCNNet: a %d x %d input leaves nothing after the trunk's 8 border pixels" % (h, w))
        ph, pw = (-h) % 4, (-w) % 4
        if not (ph or pw):
            return x
        if self.training:
            raise ValueError("VESPCNNet: a %d x %d input is not a multiple of 4 (training); eval() pads" % (h, w))
        # (plain torch indexing: not the hot path)
        rows = torch.cat([torch.arange(h), torch.full((ph,), h - 1, dtype=torch.long)]).to(x.device)
        cols = torch.cat([torch.arange(w), torch.full((pw,), w - 1, dtype=torch.long)]).to(x.device)
        return x.index_select(3, rows).index_select(4, cols)

    def forward_terms(self, x):
        h, w = x.shape[-2], x.shape[-1]
        x = self.check_image_size(x).contiguous()
        n, _, c, hp, wp = x.shape
        pair = torch.cat([x[:, 0:2].flip(1), x[:, 1:3]], 0).reshape(2 * n, 2 * c, hp, wp)   # [cur | t-1] then [cur | t+1]
        flow = self.mc(pair)
        if _training_graph(self, x):
            flow, flow_out = ops.fork(flow)
        else:
            flow_out = flow
        fused, mc = ops.motion_fuse(x, flow)
        sr = self.layers(fused)
        r = self.scale_factor
        if (hp, wp) != (h, w):
            sr = sr[:, :, :r * (h - 8), :r * (w - 8)]
        return sr, mc, flow_out

    def forward(self, x):
        return self.forward_terms(x)[0]


class FSRCNNNet(nn.Module):
    """fsrcnn.py:13-55 — note the four 3x3 mapping convs have NO activation between them and are
    followed by one bare PReLU (`mid_part.5`)."""

    def __init__(self, num_channels, scale_factor, d, s, m):
        super(FSRCNNNet, self).__init__()
        self.first_part = ConvBlock(num_channels, d, 5, 1, 0, activation='prelu', norm=None)
        self.layers = [ConvBlock(d, s, 1, 1, 0, activation='prelu', norm=None)]
        for _ in range(m):
            self.layers.append(ConvBlock(s, s, 3, 1, 1, activation=None, norm=None))
        self.layers.append(PReLU())
        self.layers.append(ConvBlock(s, d, 1, 1, 0, activation='prelu', norm=None))
        self.mid_part = nn.Sequential(*self.layers)
        self.last_part = ConvTranspose2d(d, num_channels, 9, scale_factor, 3, output_padding=1)

    def forward(self, x):
        return self.last_part(self.mid_part(self.first_part(x)))

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(mean, std)
                if m.bias is not None:
                    m.bias.data.zero_()
            if isinstance(m, nn.ConvTranspose2d):
                m.weight.data.normal_(0.0, 0.0001)
                if m.bias is not None:
                    m.bias.data.zero_()


class VDSRNet(nn.Module):
    """vdsr.py:13-36 — bias-free 3x3 stack + global residual (fused into output_conv's store)."""

    def __init__(self, num_channels, base_filter, num_residuals):
        super(VDSRNet, self).__init__()
        self.input_conv = ConvBlock(num_channels, base_filter, 3, 1, 1, norm=None, bias=False)
        self.residual_layers = nn.Sequential(*[ConvBlock(base_filter, base_filter, 3, 1, 1, norm=None, bias=False)
                                               for _ in range(num_residuals)])
        self.output_conv = ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None, bias=False)
        self.output_conv.conv._linear_tail = True   # only the global residual add lies between it and the loss (ops.py)

    def forward(self, x):
        out = self.residual_layers(self.input_conv(x))
        return self.output_conv(out, residual=x)

    def weight_init(self):
        for m in self.modules():
            utils.weights_init_kaming(m)


class DRCNNet(nn.Module):
    """drcn.py:13-59 — embedding (two 3x3 conv + ReLU), ONE conv + ReLU applied `num_recursions` times, ONE two-conv
    reconstruction applied to every hidden state, and the learnable combine weights `w` (a plain tensor that requires
    grad: not a parameter, not in the state_dict, moved by .to()).  The recursion runs into one stacked buffer
    (ops.recursive_conv) and the reconstruction on the stacked batch D*N; forward returns (list of the D y_d views,
    out = x + sum_d w_d y_d / sum w), both differentiable (to every y_d and to w) when autograd records.  The package's
    trainer takes `reconstructions` and the fused loss head instead (trainers.drcn_step)."""

    def __init__(self, num_channels, base_filter, num_recursions):
        super(DRCNNet, self).__init__()
        self.num_recursions = num_recursions
        self.embedding_layer = nn.Sequential(
            ConvBlock(num_channels, base_filter, 3, 1, 1, norm=None),
            ConvBlock(base_filter, base_filter, 3, 1, 1, norm=None))
        self.conv_block = ConvBlock(base_filter, base_filter, 3, 1, 1, norm=None)
        self.reconstruction_layer = nn.Sequential(
            ConvBlock(base_filter, base_filter, 3, 1, 1, activation=None, norm=None),
            ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None))
        # only the linear combine and the MSE terms lie between the reconstruction convs and the loss (see VDSRNet)
        for m in self.reconstruction_layer:
            m.conv._linear_tail = True
        self.w = (torch.ones(num_recursions) / num_recursions).requires_grad_(True)

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() move parameters and buffers; w is neither (drcn.py:35-36), so it is moved here
        out = super(DRCNNet, self)._apply(fn, *args, **kwargs)
        with torch.no_grad():
            w = fn(self.w)
        if w is not self.w:
            self.w = w.detach().requires_grad_(True)
        return out

    def weight_init(self):
        for m in self.modules():
            utils.weights_init_kaming(m)

    def reconstructions(self, x):
        """The D reconstructions stacked along the batch axis: [D*N, C, H, W] (y_d = rows d*N .. (d+1)*N-1)."""
        from .layers import _plan_views, grad_mode
        h0 = self.embedding_layer(x)
        c = self.conv_block.conv
        cfg = ops.ConvCfg(c._s, c._p)
        if grad_mode(h0, c.weight, c.bias):
            packed = _plan_views(c, 0)
        else:
            packed = c._cache.get(c.weight, c.bias, False, 0)
        h = ops.recursive_conv(h0, c.weight, c.bias, self.num_recursions, cfg, packed)
        return self.reconstruction_layer(h)

    def forward(self, x):
        y = self.reconstructions(x)
        n = y.shape[0] // self.num_recursions
        y_d = [y[d * n:(d + 1) * n] for d in range(self.num_recursions)]
        return y_d, ops.drcn_head(y, x, self.w)


def _trunk_with_skip(head_out, trunk, mid_conv, training):
    """out = mid_conv(trunk(h)) + h   (edsr.py:37-42, srgan.py:34-39)"""
    if training:
        h, skip = ops.fork(head_out)
    else:
        h = skip = head_out
    return mid_conv(trunk(h), residual=skip)


class EDSRNet(nn.Module):
    """edsr.py:13-45 — 16 BN-free ResnetBlocks, 2x pixel-shuffle upsamplers, L1-trained."""

    def __init__(self, num_channels, base_filter, num_residuals):
        super(EDSRNet, self).__init__()
        self.input_conv = ConvBlock(num_channels, base_filter, 3, 1, 1, activation=None, norm=None)
        self.residual_layers = nn.Sequential(*[ResnetBlock(base_filter, norm=None) for _ in range(num_residuals)])
        self.mid_conv = ConvBlock(base_filter, base_filter, 3, 1, 1, activation=None, norm=None)
        self.upscale4x = nn.Sequential(
            Upsample2xBlock(base_filter, base_filter, upsample='ps', activation=None, norm=None),
            Upsample2xBlock(base_filter, base_filter, upsample='ps', activation=None, norm=None))
        self.output_conv = ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None)
        # nothing but additions, pixel shuffles and convolutions lies between these layers' outputs and the loss: no
        # activation mask depends on their rounding, so their training forward takes the bf16x3 products of the
        # backward pass (the ReLU-carrying body keeps the fp32-faithful bf16x6; ops.set_precision("bf16x6") keeps it
        # everywhere)
        for m in (self.mid_conv.conv, self.upscale4x[0].upsample.conv, self.upscale4x[1].upsample.conv,
                  self.output_conv.conv):
            m._linear_tail = True

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)

    def forward(self, x):
        out = _trunk_with_skip(self.input_conv(x), self.residual_layers, self.mid_conv, _training_graph(self, x))
        return self.output_conv(self.upscale4x(out))


class RCANNet(nn.Module):
    """RCAN (Zhang et al., ECCV 2018; not in the reference collection): EDSR's BN-free trunk with a channel-attention gate in
    every block, residual in residual -- `num_groups` groups of `num_blocks` RCABs and a conv under a group skip, a conv
    under the long skip, log2(scale) 2x pixel-shuffle upsamplers.  No mean shift, as in this package's EDSR."""

    def __init__(self, num_channels, base_filter=64, num_groups=10, num_blocks=20, reduction=16, scale_factor=4):
        super(RCANNet, self).__init__()
        if scale_factor not in (2, 4, 8):
            raise ValueError("RCANNet: scale_factor %r is not 2, 4 or 8" % (scale_factor,))
        if num_groups < 1 or num_blocks < 1:
            raise ValueError("RCANNet: num_groups %r and num_blocks %r must be at least 1" % (num_groups, num_blocks))
        self.input_conv = ConvBlock(num_channels, base_filter, 3, 1, 1, activation=None, norm=None)
        self.residual_groups = nn.Sequential(*[ResidualGroup(base_filter, num_blocks, reduction)
                                               for _ in range(num_groups)])
        self.mid_conv = ConvBlock(base_filter, base_filter, 3, 1, 1, activation=None, norm=None)
        self.upscale = nn.Sequential(*[Upsample2xBlock(base_filter, base_filter, upsample='ps', activation=None, norm=None)
                                       for _ in range(int(math.log2(scale_factor)))])
        self.output_conv = ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None)
        # as in EDSRNet: only convolutions, additions and pixel shuffles lie between these layers and the loss
        for m in [self.mid_conv.conv, self.output_conv.conv] + [u.upsample.conv for u in self.upscale]:
            m._linear_tail = True

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)

    def forward(self, x):
        out = _trunk_with_skip(self.input_conv(x), self.residual_groups, self.mid_conv, _training_graph(self, x))
        return self.output_conv(self.upscale(out))


class RDNNet(nn.Module):
    """RDN (Zhang et al., CVPR 2018; not in the reference collection): two shallow-feature convs, D residual dense blocks
    whose outputs are all fused by a 1x1 and a 3x3 conv (GFF) under the SFENet1 skip, a pixel-shuffle upsampler.  Module
    names as in the official net (SFENet1, SFENet2, RDBs, GFF, UPNet).  The D blocks run as ONE op on channel slices
    (ops.residual_dense_blocks): its result is the buffer GFF reads, no concatenation exists anywhere in the net."""

    def __init__(self, num_channels, G0=64, D=16, C=8, G=64, scale_factor=4):
        super(RDNNet, self).__init__()
        if scale_factor not in (2, 3, 4):
            raise ValueError("RDNNet: scale_factor %r is not 2, 3 or 4" % (scale_factor,))
        if D < 1:
            raise ValueError("RDNNet: D = %r blocks, at least 1" % (D,))
        self.scale_factor = scale_factor
        self.SFENet1 = Conv2d(num_channels, G0, 3, 1, 1)
        self.SFENet2 = Conv2d(G0, G0, 3, 1, 1)
        self.RDBs = nn.ModuleList([RDB(G0, G, C) for _ in range(D)])    # (RDB raises for the G0, G and C it refuses)
        self.GFF = nn.Sequential(Conv2d(D * G0, G0, 1, 1, 0), Conv2d(G0, G0, 3, 1, 1))
        if scale_factor == 4:
            up = [Conv2d(G0, G * 4, 3, 1, 1), PixelShuffle(2), Conv2d(G, G * 4, 3, 1, 1), PixelShuffle(2)]
        else:
            r = scale_factor
            up = [Conv2d(G0, G * r * r, 3, 1, 1), PixelShuffle(r)]
        self.UPNet = nn.Sequential(*(up + [Conv2d(G, num_channels, 3, 1, 1)]))
        for conv, nxt in zip(self.UPNet, list(self.UPNet)[1:] + [None]):
            if isinstance(nxt, PixelShuffle):
                conv._ps_r = int(nxt.upscale_factor)      # the shuffle is fused into this conv's store (optim.PackPlan packs for it)
        # only convolutions, additions and pixel shuffles lie between these layers and the loss (as in EDSRNet)
        for m in list(self.GFF) + [m for m in self.UPNet if isinstance(m, Conv2d)]:
            m._linear_tail = True

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)

    def forward(self, x):
        training = _training_graph(self, x)
        f1 = self.SFENet1(x)
        if training:
            f1, skip = ops.fork(f1)   # gradient fan-in summed by srk_axpby
        else:
            skip = f1
        fusion = ops.residual_dense_blocks(self.SFENet2(f1), [b.block_params() for b in self.RDBs])
        out = self.GFF[1].run(self.GFF[0](fusion), residual=skip)
        for m in self.UPNet:
            if isinstance(m, Conv2d):
                out = m.run(out, ps_r=getattr(m, "_ps_r", 0))
        return out


class RRDBNet(nn.Module):
    """ESRGAN's generator (Wang et al., ECCV-W 2018; not in the reference collection): conv_first, nb residual-in-residual
    dense blocks, conv_body under the conv_first skip, two nearest-neighbour x2 upsamplings each followed by a conv with
    LeakyReLU(0.2), conv_hr with LeakyReLU and conv_last.  Parameter names as in BasicSR's RRDBNet (conv_first,
    body.{i}.rdb{1,2,3}.conv{1..5}, conv_body, conv_up1, conv_up2, conv_hr, conv_last).  The nb blocks run as ONE op on
    channel slices (ops.rrdb_trunk).  Scale 4 only: BasicSR's x2 goes through a pixel-unshuffle, which is not built."""

    def __init__(self, num_channels, nf=64, nb=23, gc=32, scale_factor=4):
        super(RRDBNet, self).__init__()
        if scale_factor != 4:
            raise ValueError("RRDBNet: scale_factor %r is not 4 (the only scale this net is built for)" % (scale_factor,))
        if nb < 1:
            raise ValueError("RRDBNet: nb = %r blocks, at least 1" % (nb,))
        self.scale_factor = scale_factor
        self.conv_first = Conv2d(num_channels, nf, 3, 1, 1)
        self.body = nn.ModuleList([RRDB(nf, gc) for _ in range(nb)])     # (RRDB raises for the nf and gc it refuses)
        self.conv_body = Conv2d(nf, nf, 3, 1, 1)
        self.conv_up1 = Conv2d(nf, nf, 3, 1, 1)
        self.conv_up2 = Conv2d(nf, nf, 3, 1, 1)
        self.conv_hr = Conv2d(nf, nf, 3, 1, 1)
        self.conv_last = Conv2d(nf, num_channels, 3, 1, 1)
        self.conv_last._linear_tail = True

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)

    def forward(self, x):
        training = _training_graph(self, x)
        feat = self.conv_first(x)
        if training:
            feat, skip = ops.fork(feat)   # gradient fan-in summed by srk_axpby
        else:
            skip = feat
        trunk = ops.rrdb_trunk(feat, [b.block_params() for b in self.body], self.body[0].res_scale)
        out = self.conv_body.run(trunk, residual=skip)
        out = self.conv_up1.run(ops.upsample_nearest(out, 2), ACT_LRELU, 0.2)
        out = self.conv_up2.run(ops.upsample_nearest(out, 2), ACT_LRELU, 0.2)
        return self.conv_last.run(self.conv_hr.run(out, ACT_LRELU, 0.2))


class _PatchEmbed(nn.Module):
    """Upstream's `patch_embed` at patch size 1: only its LayerNorm has parameters (`patch_embed.norm.*`)."""

    def __init__(self, dim):
        super(_PatchEmbed, self).__init__()
        self.norm = LayerNorm(dim)

    def forward(self, x):
        return self.norm(x)


SWINIR_RGB_MEAN = (0.4488, 0.4371, 0.4040)
SWINIR_UPSAMPLERS = ("pixelshuffle", "pixelshuffledirect")


class SwinIRNet(nn.Module):
    """SwinIR (Liang et al., ICCVW 2021; not in the reference collection), the classical (`pixelshuffle`) and lightweight
    (`pixelshuffledirect`) image-SR nets: mean shift for 3 channels, conv_first, patch_embed.norm, `len(depths)` RSTBs
    (layers.{i}.residual_group.blocks.{j}.*, layers.{i}.conv), norm, conv_after_body under the long skip, the upsampler.
    Module names follow upstream's network_swinir.py as remembered; they could not be checked against it.  Upstream's
    `relative_position_index` and `attn_mask` buffers do not exist (the attention kernel computes both), so an upstream
    checkpoint loads with strict=False.  Not built: stochastic depth (upstream's class default drop_path_rate = 0.1),
    the absolute position embedding, resi_connection = '3conv', the real-SR 'nearest+conv' upsampler.
    A token is an NHWC pixel: the map never leaves its layout, the projections are 1x1 convolutions."""

    def __init__(self, num_channels, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=6, window_size=8, mlp_ratio=2,
                 scale_factor=4, upsampler="pixelshuffle"):
        super(SwinIRNet, self).__init__()
        if upsampler not in SWINIR_UPSAMPLERS:
            raise ValueError("SwinIRNet: upsampler %r is not one of %s" % (upsampler, SWINIR_UPSAMPLERS))
        if upsampler == "pixelshuffle" and scale_factor not in (2, 3, 4, 8):
            raise ValueError("SwinIRNet: scale_factor %r is not 2, 3, 4 or 8 (pixelshuffle)" % (scale_factor,))
        if int(scale_factor) < 1:
            raise ValueError("SwinIRNet: scale_factor %r" % (scale_factor,))
        depths = tuple(int(d) for d in depths)
        if not depths or min(depths) < 1:
            raise ValueError("SwinIRNet: depths %r, at least one RSTB of at least one layer" % (depths,))
        ops.window_attention_check(embed_dim, num_heads, window_size, window_size // 2, who="SwinIRNet")
        self.window_size, self.scale_factor, self.upsampler = int(window_size), int(scale_factor), upsampler
        self.mean = SWINIR_RGB_MEAN if num_channels == 3 else None
        self.conv_first = Conv2d(num_channels, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim)
        self.layers = nn.ModuleList([RSTB(embed_dim, d, num_heads, window_size, mlp_ratio) for d in depths])
        self.norm = LayerNorm(embed_dim)
        self.conv_after_body = Conv2d(embed_dim, embed_dim, 3, 1, 1)
        if upsampler == "pixelshuffle":
            num_feat = 64
            self.conv_before_upsample = nn.Sequential(Conv2d(embed_dim, num_feat, 3, 1, 1), LeakyReLU(inplace=True))
            up = []
            if scale_factor == 3:
                up = [Conv2d(num_feat, 9 * num_feat, 3, 1, 1), PixelShuffle(3)]
            else:
                for _ in range(int(math.log2(scale_factor))):
                    up += [Conv2d(num_feat, 4 * num_feat, 3, 1, 1), PixelShuffle(2)]
            self.upsample = nn.Sequential(*up)
            self.conv_last = Conv2d(num_feat, num_channels, 3, 1, 1)
        else:
            self.upsample = nn.Sequential(Conv2d(embed_dim, scale_factor ** 2 * num_channels, 3, 1, 1),
                                          PixelShuffle(scale_factor))
        for conv, nxt in zip(self.upsample, list(self.upsample)[1:] + [None]):
            if isinstance(nxt, PixelShuffle):
                conv._ps_r = int(nxt.upscale_factor)      # the shuffle is fused into this conv's store (optim.PackPlan)

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)

    def check_image_size(self, x):
        """Training: the LR size must be a multiple of the window.  eval(): reflect padding at the bottom and the right up
        to the next multiple (plain torch indexing: not the hot path)."""
        h, w = x.shape[2], x.shape[3]
        ph, pw = (-h) % self.window_size, (-w) % self.window_size
        if not (ph or pw):
            return x
        if self.training:
            raise ValueError("SwinIRNet: a %d x %d input is not a multiple of the window %d (training); eval() pads"
                             % (h, w, self.window_size))
        if ph >= h or pw >= w:
            raise ValueError("SwinIRNet: a %d x %d input cannot be reflect-padded to a multiple of the window %d"
                             % (h, w, self.window_size))
        if ph:
            x = torch.cat([x, x[:, :, h - 1 - ph:h - 1].flip(2)], 2)
        if pw:
            x = torch.cat([x, x[:, :, :, w - 1 - pw:w - 1].flip(3)], 3)
        return x

    def forward(self, x):
        h, w = x.shape[2], x.shape[3]
        x = self.check_image_size(x)
        if self.mean is not None:
            x = ops.channel_affine(x, self.mean, (1.0, 1.0, 1.0))
        first = self.conv_first(x)
        training = _training_graph(self, x)
        if training:
            first, skip = ops.fork(first)   # gradient fan-in summed by srk_axpby
        else:
            skip = first
        t = self.patch_embed(first)
        for layer in self.layers:
            t = layer(t)
        out = self.conv_after_body.run(self.norm(t), residual=skip)
        if self.upsampler == "pixelshuffle":
            out = self.conv_before_upsample[0].run(out, ACT_LRELU, self.conv_before_upsample[1].slope)
            for m in self.upsample:
                if isinstance(m, Conv2d):
                    out = m.run(out, ps_r=m._ps_r)
            out = self.conv_last(out)
        else:
            out = self.upsample[0].run(out, ps_r=self.upsample[0]._ps_r)
        if self.mean is not None:
            out = ops.channel_affine(out, tuple(-v for v in self.mean), (1.0, 1.0, 1.0))
        if out.shape[2] != h * self.scale_factor or out.shape[3] != w * self.scale_factor:
            out = out[:, :, :h * self.scale_factor, :w * self.scale_factor]
        return out


def get_upsample_filter(size):
    """lapsrn.py:14-24 — 2-D bilinear kernel."""
    factor = (size + 1) // 2
    center = factor - 1 if size % 2 == 1 else factor - 0.5
    og = np.ogrid[:size, :size]
    filt = (1 - abs(og[0] - center) / factor) * (1 - abs(og[1] - center) / factor)
    return torch.from_numpy(filt).float()


class LapSRNNet(nn.Module):
    """lapsrn.py:27-72 — two pyramid levels that SHARE the feature branch modules
    (`convt_F1` and `convt_F2` are Sequentials over the same block objects)."""

    def __init__(self, num_channels, base_filter, num_convs):
        super(LapSRNNet, self).__init__()
        self.input_conv = ConvBlock(num_channels, base_filter, 3, 1, 1, activation='lrelu', norm=None, bias=False)
        conv_blocks = [ConvBlock(base_filter, base_filter, 3, 1, 1, activation='lrelu', norm=None, bias=False)
                       for _ in range(num_convs)]
        conv_blocks.append(DeconvBlock(base_filter, base_filter, 4, 2, 1, activation='lrelu', norm=None, bias=False))
        self.convt_I1 = DeconvBlock(num_channels, num_channels, 4, 2, 1, activation=None, norm=None, bias=False)
        self.convt_R1 = ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None, bias=False)
        self.convt_F1 = nn.Sequential(*conv_blocks)
        self.convt_I2 = DeconvBlock(num_channels, num_channels, 4, 2, 1, activation=None, norm=None, bias=False)
        self.convt_R2 = ConvBlock(base_filter, num_channels, 3, 1, 1, activation=None, norm=None, bias=False)
        self.convt_F2 = nn.Sequential(*conv_blocks)

    def weight_init(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
                if m.bias is not None:
                    m.bias.data.zero_()
            if isinstance(m, nn.ConvTranspose2d):
                c1, c2, h, w = m.weight.data.size()
                m.weight.data.copy_(get_upsample_filter(h).view(1, 1, h, w).repeat(c1, c2, 1, 1))
                if m.bias is not None:
                    m.bias.data.zero_()

    def forward(self, x):
        training = _training_graph(self, x)
        out = self.input_conv(x)
        f1 = self.convt_F1(out)
        if training:
            f1a, f1b = ops.fork(f1)
        else:
            f1a = f1b = f1
        i1 = self.convt_I1(x)
        x_coarse = self.convt_R1(f1a, residual=i1)
        if training:
            xc_out, xc_in = ops.fork(x_coarse)
        else:
            xc_out = xc_in = x_coarse
        f2 = self.convt_F2(f1b)
        i2 = self.convt_I2(xc_in)
        x_finer = self.convt_R2(f2, residual=i2)
        return xc_out, x_finer


class SRGANGenerator(nn.Module):
    """srgan.py:14-46 — SRResNet: 9x9 head, 16 ResnetBlocks (shared BN + PReLU each), BN'd mid conv,
    2x PS+PReLU upsamplers, 9x9 tail."""

    def __init__(self, num_channels, base_filter, num_residuals):
        super(SRGANGenerator, self).__init__()
        self.input_conv = ConvBlock(num_channels, base_filter, 9, 1, 4, activation='prelu', norm=None)
        self.residual_layers = nn.Sequential(*[ResnetBlock(base_filter, activation='prelu')
                                               for _ in range(num_residuals)])
        self.mid_conv = ConvBlock(base_filter, base_filter, 3, 1, 1, activation=None)
        self.upscale4x = nn.Sequential(
            Upsample2xBlock(base_filter, base_filter, upsample='ps', activation='prelu', norm=None),
            Upsample2xBlock(base_filter, base_filter, upsample='ps', activation='prelu', norm=None))
        self.output_conv = ConvBlock(base_filter, num_channels, 9, 1, 4, activation=None, norm=None)

    def forward(self, x):
        out = _trunk_with_skip(self.input_conv(x), self.residual_layers, self.mid_conv, _training_graph(self, x))
        return self.output_conv(self.upscale4x(out))

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)


class SRGANDiscriminator(nn.Module):
    """srgan.py:49-81 — 8 convs (stride 1/2 alternating, BN + LeakyReLU) + 2 dense layers."""

    def __init__(self, num_channels, base_filter, image_size):
        super(SRGANDiscriminator, self).__init__()
        self.image_size = image_size
        self.input_conv = ConvBlock(num_channels, base_filter, 3, 1, 1, activation='lrelu', norm=None)
        self.conv_blocks = nn.Sequential(
            ConvBlock(base_filter, base_filter, 3, 2, 1, activation='lrelu'),
            ConvBlock(base_filter, base_filter * 2, 3, 1, 1, activation='lrelu'),
            ConvBlock(base_filter * 2, base_filter * 2, 3, 2, 1, activation='lrelu'),
            ConvBlock(base_filter * 2, base_filter * 4, 3, 1, 1, activation='lrelu'),
            ConvBlock(base_filter * 4, base_filter * 4, 3, 2, 1, activation='lrelu'),
            ConvBlock(base_filter * 4, base_filter * 8, 3, 1, 1, activation='lrelu'),
            ConvBlock(base_filter * 8, base_filter * 8, 3, 2, 1, activation='lrelu'))
        self.dense_layers = nn.Sequential(
            DenseBlock(base_filter * 8 * image_size // 16 * image_size // 16, base_filter * 16, activation='lrelu',
                       norm=None),
            DenseBlock(base_filter * 16, 1, activation='sigmoid', norm=None))

    def forward(self, x):
        out = self.conv_blocks(self.input_conv(x))
        out = ops.flatten_nchw(out)  # out.view(B, -1) in (C,H,W) order, srgan.py:75
        return self.dense_layers(out)

    def weight_init(self, mean=0.0, std=0.02):
        for m in self.modules():
            utils.weights_init_normal(m, mean=mean, std=std)


class ESRGANDiscriminator(SRGANDiscriminator):
    """SRGANDiscriminator's body ending in a LOGIT: the last dense layer has no sigmoid, as the relativistic average loss
    (ops.ragan_loss) takes it.  (BasicSR's 4x4 stride-2 VGG-style discriminator is not built.)"""

    def __init__(self, num_channels, base_filter, image_size):
        super(ESRGANDiscriminator, self).__init__(num_channels, base_filter, image_size)
        self.dense_layers = nn.Sequential(
            DenseBlock(base_filter * 8 * image_size // 16 * image_size // 16, base_filter * 16, activation='lrelu',
                       norm=None),
            DenseBlock(base_filter * 16, 1, activation=None, norm=None))


class UNetDiscriminatorSN(nn.Module):
    """Real-ESRGAN's U-Net discriminator with spectral normalisation (Wang et al., ICCVW 2021; not in the reference
    collection), under the names its checkpoints carry: conv0 (3x3, bias), conv1..3 (4x4 stride 2), conv4..6 (3x3 behind a
    bilinear x2), conv7, conv8 (3x3), all bias-free under spectral norm (`weight_orig`, `weight_u`, `weight_v`), conv9
    (3x3 to one channel, bias).  Leaky ReLU 0.2 in every conv's epilogue but the last; skips x4 += x2, x5 += x1, x6 += x0.
    Fully convolutional: [B, C, H, W] -> [B, 1, H, W] logits for H and W multiples of 8; no BatchNorm.
    All eight normalised filters come from ONE ops.spectral_norm call at the top of forward (three launches); two skip
    additions ride in the next upsample's read (ops.upsample_bilinear2x(add=)), the third is ops.add."""

    SN_LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8")

    def __init__(self, num_in_ch=3, num_feat=64, skip_connection=True):
        super(UNetDiscriminatorSN, self).__init__()
        from .layers import SpectralNormConv2d as SN
        f = int(num_feat)
        self.num_in_ch, self.num_feat, self.skip_connection = int(num_in_ch), f, bool(skip_connection)
        self.conv0 = Conv2d(num_in_ch, f, 3, 1, 1)
        self.conv1 = SN(f, 2 * f, 4, 2, 1)
        self.conv2 = SN(2 * f, 4 * f, 4, 2, 1)
        self.conv3 = SN(4 * f, 8 * f, 4, 2, 1)
        self.conv4 = SN(8 * f, 4 * f, 3, 1, 1)
        self.conv5 = SN(4 * f, 2 * f, 3, 1, 1)
        self.conv6 = SN(2 * f, f, 3, 1, 1)
        self.conv7 = SN(f, f, 3, 1, 1)
        self.conv8 = SN(f, f, 3, 1, 1)
        self.conv9 = Conv2d(f, 1, 3, 1, 1)

    def weight_init(self, mean=0.0, std=0.02):
        """Real-ESRGAN trains this net from torch's default initialisation, which the constructors have already drawn."""
        return None

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.num_in_ch:
            raise ValueError("UNetDiscriminatorSN: takes [B, %d, H, W], got shape %s" % (self.num_in_ch, tuple(x.shape)))
        for name, v in (("H", x.shape[2]), ("W", x.shape[3])):
            if v % 8 or v < 8:
                raise ValueError("UNetDiscriminatorSN: %s = %d is not a multiple of 8 (three stride-2 stages)" % (name, v))
        lrelu = dict(act=ACT_LRELU, slope=0.2)
        training = _training_graph(self, x)
        w = ops.spectral_norm([getattr(self, n).spectral_layer() for n in self.SN_LAYERS], self.training)
        split = ops.fork if (training and self.skip_connection) else (lambda t: (t, t))
        x0, s0 = split(self.conv0.run(x, **lrelu))
        x1, s1 = split(self.conv1.run(x0, w[0], **lrelu))
        x2, s2 = split(self.conv2.run(x1, w[1], **lrelu))
        x3 = self.conv3.run(x2, w[2], **lrelu)
        skip = self.skip_connection
        x4 = self.conv4.run(ops.upsample_bilinear2x(x3), w[3], **lrelu)
        x5 = self.conv5.run(ops.upsample_bilinear2x(x4, s2 if skip else None), w[4], **lrelu)
        x6 = self.conv6.run(ops.upsample_bilinear2x(x5, s1 if skip else None), w[5], **lrelu)
        if skip:
            x6 = ops.add(x6, s0)
        out = self.conv7.run(x6, w[6], **lrelu)
        out = self.conv8.run(out, w[7], **lrelu)
        return self.conv9.run(out)


class _MaxPool2x2(nn.MaxPool2d):
    """nn.MaxPool2d(kernel_size=2, stride=2) surface (vgg19.features[4]) on srk_maxpool2x2_forward."""

    def __init__(self):
        super(_MaxPool2x2, self).__init__(kernel_size=2, stride=2)

    def forward(self, x):
        return ops.max_pool2x2(x)


class FeatureExtractor(nn.Module):
    """srgan.py:84-90 — `nn.Sequential(*list(vgg19.features.children())[:feature_layer + 1])`: for the reference's
    feature_layer = 8 that is conv3-64, ReLU, conv64-64, ReLU, MaxPool 2x2, conv64-128, ReLU, conv128-128, ReLU, kept
    under the same indices so a torchvision `vgg19` checkpoint's `features.{0,2,5,7}.{weight,bias}` load directly
    (`load_vgg19`).  The reference downloads pretrained weights (srgan.py:144); without network access the weights
    are whatever the caller loads (kaiming-normal until then, like torchvision's own init).  forward() evaluates the
    module without gradients, as the reference does (srgan.py:302-305); extract(x, grad=True) is the same walk
    differentiable in x, for a perceptual loss that trains (ops.perceptual_loss).  conv + ReLU run as one fused kernel each."""

    # torchvision.models.vgg19 `features` layout up to index 36: numbers = conv3x3 output channels, 'M' = MaxPool2d(2,2)
    VGG19_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M')

    def __init__(self, netVGG=None, feature_layer=8):
        super(FeatureExtractor, self).__init__()
        from .layers import Conv2d, ReLU
        mods, cin = [], 3
        for v in self.VGG19_CFG:
            if v == 'M':
                mods.append(_MaxPool2x2())
            else:
                mods += [Conv2d(cin, v, 3, 1, 1), ReLU(True)]
                cin = v
        self.features = nn.Sequential(*mods[:feature_layer + 1])
        for m in self.features:
            if isinstance(m, nn.Conv2d):   # torchvision's VGG initialisation
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                m.bias.data.zero_()
        for p in self.parameters():
            p.requires_grad_(False)
        for m in self.features:
            if isinstance(m, nn.Conv2d):   # in no optimizer: the packs outlive optimizer steps (layers._PackCache)
                m._cache.frozen = True
        if netVGG is not None:
            self.load_vgg19(netVGG.state_dict() if hasattr(netVGG, "state_dict") else netVGG)

    def load_vgg19(self, state_dict):
        """Copy `features.N.weight/bias` of a torchvision vgg19 state_dict (or a path to its .pth file) for the
        layers this extractor keeps; classifier / deeper feature entries are ignored."""
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location="cpu")
        own = self.state_dict()
        picked = {k: v for k, v in state_dict.items() if k in own}
        missing = [k for k in own if k not in picked]
        if missing:
            raise KeyError("vgg19 state_dict lacks %s" % missing)
        self.load_state_dict(picked)
        from .layers import bump_weight_epoch
        bump_weight_epoch()
        for m in self.features:
            if isinstance(m, nn.Conv2d):
                m._cache.drop()
        return self

    def forward(self, x):
        return self.extract(x, grad=False)

    def extract(self, x, grad=False):
        """The walk through the head: conv + ReLU as one fused kernel each, the pools in between.
        grad=False: on the detached input, without a graph, on the inference kernels -- the reference's use.
        grad=True: differentiable with respect to x (ops.perceptual_loss): the convs run ops.conv2d (the training forward,
        in grad mode or not: both operands of the loss then see the same kernels), the pools ops.max_pool2x2_train.  The
        parameters stay frozen, so a backward pass runs data gradients only, and both filter packs of every layer come
        from the layer's cache: a train step launches no pack for the head."""
        if not grad:
            with torch.no_grad():
                return self._walk(x.detach(), False)
        return self._walk(x, True)

    def _walk(self, out, grad):
        return _vgg_walk(list(self.features), out, grad)

    def tap_walk(self, a, b, taps):
        """The multi-layer feature term of ops.vgg_feature_loss on already normalised operands: see _vgg_pair_walk."""
        return _vgg_pair_walk(list(self.features), a, b, taps)


def _vgg_modules(cfg):
    """torchvision's `features` of a VGG configuration (numbers = conv3x3 output channels, 'M' = MaxPool2d(2,2)) as this
    package's modules, under torchvision's indices, with torchvision's initialisation."""
    from .layers import Conv2d, ReLU
    mods, cin = [], 3
    for v in cfg:
        if v == 'M':
            mods.append(_MaxPool2x2())
        else:
            conv = Conv2d(cin, v, 3, 1, 1)
            nn.init.kaiming_normal_(conv.weight, mode='fan_out', nonlinearity='relu')
            conv.bias.data.zero_()
            mods += [conv, ReLU(True)]
            cin = v
    return mods


def _freeze_vgg(module):
    """No parameter of a VGG head trains, and its convs are in no optimizer: their packs outlive optimizer steps
    (layers._PackCache)."""
    for p in module.parameters():
        p.requires_grad_(False)
    for m in module.features:
        if isinstance(m, nn.Conv2d):
            m._cache.frozen = True


def _load_vgg_features(module, state_dict, what):
    """Copy `features.N.weight/bias` of a torchvision VGG state_dict (or a path to its .pth file) for the layers `module`
    keeps; every other entry is ignored, a missing one is a KeyError."""
    if isinstance(state_dict, str):
        state_dict = torch.load(state_dict, map_location="cpu")
    own = [k for k in module.state_dict() if k.startswith("features.")]
    missing = [k for k in own if k not in state_dict]
    if missing:
        raise KeyError("%s state_dict lacks %s" % (what, missing))
    module.load_state_dict({k: state_dict[k] for k in own}, strict=False)
    from .layers import bump_weight_epoch
    bump_weight_epoch()
    for m in module.features:
        if isinstance(m, nn.Conv2d):
            m._cache.drop()
    return module


def _vgg_walk(mods, out, grad, taps=None):
    """The walk through a VGG head given as its module list: conv + ReLU as one fused kernel each, the pools in between
    (FeatureExtractor.extract says what `grad` chooses).  taps=None: returns the last map.  taps = module indices:
    returns the list of the maps that leave those modules (a fused ReLU's index for a conv + ReLU pair); where autograd
    records, a tapped map that the walk goes on from is forked (ops.fork: it feeds its consumer here and the next layer
    there, and the two gradients are added by srk_axpby)."""
    got = []
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Conv2d):
            fused = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            act = ACT_RELU if fused else ACT_NONE
            if grad:
                out = ops.conv2d(out, m.weight, m.bias, None, ops.ConvCfg(m._s, m._p, False, 0, act),
                                 m._cache.get(m.weight, m.bias, False, 0, bwd=True))
            else:
                out = m.run(out, act)   # conv + bias + ReLU in one kernel
            i += 2 if fused else 1
        elif isinstance(m, _MaxPool2x2) and grad:
            out = ops.max_pool2x2_train(out)
            i += 1
        else:
            out = m(out)
            i += 1
        if taps is not None and i - 1 in taps:
            if i < len(mods) and ops.grad_enabled_for(out):
                keep, out = ops.fork(out)
            else:
                keep = out
            got.append(keep)
    return out if taps is None else got


def _vgg_pair_walk(mods, a, b, taps):
    """Prediction `a` and target `b` through a VGG head in lockstep, up to the deepest tap; taps = [(conv index, weight)]
    in the order of the head.  Returns sum_k weight_k * L1 of the two maps that leave conv k BEFORE its ReLU
    (ops.vgg_feature_loss).  Untapped layers run as _vgg_walk(grad=True) runs them, `b` without a graph on the same
    kernels.  A tapped conv runs without its ReLU, both packs from the layer's cache, and ops.vgg_tap then does in one
    launch what the head runs behind it: the ReLU and the pool, the ReLU alone, or nothing at the deepest tap -- no fork,
    no separate ReLU or pool launch."""
    want = dict(taps)
    last = max(want)
    ws = torch.empty(int(_lib.load().srk_vgg_tap_workspace_bytes(len(want))), dtype=torch.uint8, device=a.device)
    tokens = []
    i = 0
    while i <= last:
        m = mods[i]
        if isinstance(m, nn.Conv2d):
            fused = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            tapped = i in want
            cfg = ops.ConvCfg(m._s, m._p, False, 0, ACT_RELU if (fused and not tapped) else ACT_NONE)
            packs = m._cache.get(m.weight, m.bias, False, 0, bwd=True)
            a = ops.conv2d(a, m.weight, m.bias, None, cfg, packs)
            with torch.no_grad():
                b = ops.conv2d(b, m.weight, m.bias, None, cfg, packs)
            step = 2 if fused else 1
            if tapped:
                if i == last:
                    mode = _lib.VGG_TAP_LAST
                elif fused and i + 2 < len(mods) and isinstance(mods[i + 2], _MaxPool2x2):
                    mode, step = _lib.VGG_TAP_POOL, 3
                elif fused:
                    mode = _lib.VGG_TAP_RELU
                else:
                    raise ValueError("vgg tap: layer %d is followed by neither a ReLU nor the end of the walk" % i)
                token, a, b = ops.vgg_tap(a, b, mode, want[i], len(tokens), len(want), ws)
                tokens.append(token)
            i += step
        elif isinstance(m, _MaxPool2x2):
            a = ops.max_pool2x2_train(a)
            with torch.no_grad():
                b = ops.max_pool2x2_train(b)
            i += 1
        else:
            a, b = m(a), m(b)
            i += 1
    return ops.vgg_tap_finish(ws, len(want), tokens)


class LPIPS(nn.Module):
    """The net of LPIPS (Zhang et al. 2018), VGG variant: torchvision's vgg16.features up to index 29 (the fifth pool is
    not run), tapped behind ReLU 1_2, 2_2, 3_3, 4_3 and 5_3 (indices 3, 8, 15, 22, 29; 64, 128, 256, 512, 512 channels),
    and the five non-negative 1 x 1 weight vectors `lins`.  `features` keeps torchvision's indices, so a vgg16
    checkpoint's `features.N.weight/bias` load directly (`load_vgg16`); `load_lins` takes the `lpips` package's vgg.pth
    (`lin{l}.model.1.weight`, each [1, C_l, 1, 1]).  Until loaded: torchvision's initialisation and lins of 1 / C_l.
    Every parameter is frozen.  forward(x) / extract(x): the five maps of an already scaled input; ops.lpips(pred,
    target, net) is the metric and the loss."""

    VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
    TAPS = (3, 8, 15, 22, 29)
    WIDTHS = (64, 128, 256, 512, 512)

    def __init__(self, vgg16=None, lins=None):
        super(LPIPS, self).__init__()
        self.features = nn.Sequential(*_vgg_modules(self.VGG16_CFG))
        self.lins = nn.ParameterList([nn.Parameter(torch.full((c,), 1.0 / c)) for c in self.WIDTHS])
        _freeze_vgg(self)
        if vgg16 is not None:
            self.load_vgg16(vgg16.state_dict() if hasattr(vgg16, "state_dict") else vgg16)
        if lins is not None:
            self.load_lins(lins)

    def load_vgg16(self, state_dict):
        """Copy `features.N.weight/bias` of a torchvision vgg16 state_dict (or a path to its .pth file); classifier
        entries are ignored, a missing layer is a KeyError."""
        return _load_vgg_features(self, state_dict, "vgg16")

    def load_lins(self, state_dict):
        """Copy the five weight vectors from the `lpips` package's vgg.pth state_dict (or a path to it): exactly the keys
        `lin{l}.model.1.weight`, l = 0..4, each with C_l elements; a missing one is a KeyError."""
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location="cpu")
        keys = ["lin%d.model.1.weight" % l for l in range(len(self.WIDTHS))]
        missing = [k for k in keys if k not in state_dict]
        if missing:
            raise KeyError("lpips state_dict lacks %s" % missing)
        for k, c, p in zip(keys, self.WIDTHS, self.lins):
            v = state_dict[k]
            if v.numel() != c:
                raise ValueError("lpips state_dict: %s has %d elements, the tap has %d channels" % (k, v.numel(), c))
            p.data.copy_(v.detach().reshape(-1).to(p.dtype))
        return self

    def forward(self, x):
        return self.extract(x, grad=False)

    def extract(self, x, grad=False):
        """The five tapped maps of x (already shifted and scaled: ops.lpips_input_affine), as FeatureExtractor.extract:
        grad=False on the detached input, without a graph, on the inference kernels; grad=True the training forward,
        differentiable in x where autograd records."""
        mods = list(self.features)
        if not grad:
            with torch.no_grad():
                return _vgg_walk(mods, x.detach(), False, self.TAPS)
        return _vgg_walk(mods, x, True, self.TAPS)
