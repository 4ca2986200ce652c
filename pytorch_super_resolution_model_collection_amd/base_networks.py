"""The shared block library of the reference (base_networks.py:4-214) on the MI355X kernels.

Same six class names, constructor signatures, sub-module attribute names (`conv`, `deconv`, `fc`,
`bn`, `act`, `ps`, `upsample`) and therefore the same state_dict keys.  Each block's forward maps
to as few kernel launches as the arithmetic allows:

    ConvBlock / DeconvBlock   conv + bias + activation                     -> 1 launch
    ResnetBlock (no norm)     conv+act, conv + residual add                -> 2 launches
    PSBlock (no norm)         conv + bias + pixel-shuffle store (+ act)    -> 1 launch (+1 in training w/ PReLU)
    RCAB (RCAN; not in the reference)  conv+act, conv, channel-attention gate + residual add -> 4 launches
    SwinTransformerLayer (SwinIR; not in the reference)  norm, qkv, attention, proj + skip, norm, fc1, GELU, fc2 + skip
                                                                                  -> 8 launches
    RDB (RDN; not in the reference)    C convs + ReLU on channel slices, 1x1 fusion + skip    -> C + 1 launches, no cat

With autograd enabled only ReLU / LeakyReLU are fused into the conv (their gradient mask can be
recovered from the saved output); PReLU / tanh / sigmoid then run as a separate pointwise kernel
that saves what its backward needs.
"""
import torch

from . import ops
from .layers import (ACT_LRELU, ACT_NONE, ACT_PRELU, ACT_RELU, GELU, BatchNorm2d, Conv2d, ConvTranspose2d, GateConv2d,
                     LayerNorm, Linear, PixelShuffle, ReLU, Sigmoid, SliceConv2d, TokenLinear, _plan_views, grad_mode,
                     make_activation, make_norm1d, make_norm2d)

_FUSABLE_IN_TRAINING = (ACT_NONE, ACT_RELU, ACT_LRELU)


class _Block(torch.nn.Module):
    """Common activation / norm plumbing of the reference blocks."""

    def _setup(self, channels, activation, norm, norm1d=False):
        self.norm = norm
        bn = make_norm1d(norm, channels) if norm1d else make_norm2d(norm, channels)
        if bn is not None:
            self.bn = bn
        self.activation = activation
        act = make_activation(activation)
        if act is not None:
            self.act = act

    def _act_args(self):
        """(kind, slope, prelu_weight) of this block's activation."""
        act = getattr(self, "act", None)
        if self.activation is None or act is None:
            return ACT_NONE, 0.0, None
        return act.kind, act.slope, (act.weight if act.kind == ACT_PRELU else None)

    def _post(self, out, fused_act):
        """norm -> activation after the main op (reference order: act(bn(op(x))))."""
        if self.norm is not None:
            kind, slope, pw = self._act_args()
            if (not fused_act and kind != ACT_NONE and isinstance(self.bn, BatchNorm2d)
                    and ops.bn_fusable(out, kind, pw, self.bn)):
                return self.bn.run(out, kind, slope, pw)   # act(bn(x)) in the BatchNorm's launches
            out = self.bn(out)
        if self.activation is not None and not fused_act:
            out = self.act(out)
        return out

    def _fuse_act(self, *tensors):
        """Can the activation ride in the conv epilogue for this call?"""
        if self.norm is not None:
            return False
        kind, _, pw = self._act_args()
        if kind == ACT_NONE:
            return True
        if grad_mode(*tensors, pw):
            return kind in _FUSABLE_IN_TRAINING
        return True


class DenseBlock(_Block):
    """base_networks.py:4-36"""

    def __init__(self, input_size, output_size, bias=True, activation='relu', norm='batch'):
        super(DenseBlock, self).__init__()
        self.fc = Linear(input_size, output_size, bias=bias)
        self._setup(output_size, activation, norm, norm1d=True)

    def forward(self, x):
        kind, slope, pw = self._act_args()
        fuse = kind != ACT_PRELU and self.norm is None   # act(bn(fc(x))): the activation follows the norm
        out = self.fc.run(x, kind if fuse else ACT_NONE, slope)
        return self._post(out, fuse)


class ConvBlock(_Block):
    """base_networks.py:39-71"""

    def __init__(self, input_size, output_size, kernel_size=4, stride=2, padding=1, bias=True, activation='relu',
                 norm='batch'):
        super(ConvBlock, self).__init__()
        self.conv = Conv2d(input_size, output_size, kernel_size, stride, padding, bias=bias)
        self._setup(output_size, activation, norm)

    def forward(self, x, residual=None):
        """`residual` (not in the reference signature) lets a caller fuse `torch.add(out, residual)`
        (vdsr.py:31, edsr.py:42) into this block's kernel when the block has no activation."""
        kind, slope, pw = self._act_args()
        fuse = self._fuse_act(x, self.conv.weight, self.conv.bias, residual)
        fuse_res = residual is not None and self.norm is None and (kind == ACT_NONE or not grad_mode(
            x, self.conv.weight, self.conv.bias, residual, pw)) and fuse
        out = self.conv.run(x, kind if fuse else ACT_NONE, slope, pw if fuse else None,
                            residual if fuse_res else None)
        out = self._post(out, fuse)
        if residual is not None and not fuse_res:
            out = ops.add(out, residual)
        return out


class DeconvBlock(_Block):
    """base_networks.py:74-106"""

    def __init__(self, input_size, output_size, kernel_size=4, stride=2, padding=1, bias=True, activation='relu',
                 norm='batch'):
        super(DeconvBlock, self).__init__()
        self.deconv = ConvTranspose2d(input_size, output_size, kernel_size, stride, padding, bias=bias)
        self._setup(output_size, activation, norm)

    def forward(self, x):
        kind, slope, pw = self._act_args()
        fuse = self._fuse_act(x, self.deconv.weight, self.deconv.bias)
        out = self.deconv.run(x, kind if fuse else ACT_NONE, slope, pw if fuse else None)
        return self._post(out, fuse)


class ResnetBlock(_Block):
    """base_networks.py:109-150 — note ONE `bn` (and one `act`) shared by both convs."""

    def __init__(self, num_filter, kernel_size=3, stride=1, padding=1, bias=True, activation='relu', norm='batch'):
        super(ResnetBlock, self).__init__()
        self.conv1 = Conv2d(num_filter, num_filter, kernel_size, stride, padding, bias=bias)
        self.conv2 = Conv2d(num_filter, num_filter, kernel_size, stride, padding, bias=bias)
        self._setup(num_filter, activation, norm)

    def forward(self, x):
        kind, slope, pw = self._act_args()
        training = grad_mode(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, pw)
        if self.norm is None:
            fuse = self._fuse_act(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias)
            if (training and fuse and kind == ACT_RELU and self.conv1._s == 1 and self.conv1._p == 1
                    and self.conv2._s == 1 and self.conv2._p == 1
                    and ops.resblock2_applicable(x, self.conv1.weight, self.conv2.weight)):
                # small problems (a strong-scaled shard): both convs, the ReLU and the skip in one launch per direction
                return ops.resblock2(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                     _plan_views(self.conv1, 0), _plan_views(self.conv2, 0))
            # training: the skip gradient (= the block output gradient) is added by conv1's data-gradient kernel
            # (ops.GradBox); it needs x itself to require grad, else there is no fan-in to sum
            box = ops.GradBox() if (training and x.requires_grad and ops.FUSE_SKIP_GRAD) else None
            residual = x
            if training and box is None:
                x, residual = ops.fork(x)  # unfused: gradient fan-in summed by srk_axpby
            out = self.conv1.run(x, kind if fuse else ACT_NONE, slope, pw if fuse else None, add_box=box)
            if not fuse:
                out = self.act(out)
            return self.conv2.run(out, ACT_NONE, 0.0, None, residual, res_box=box)  # conv2 + residual add, one kernel
        fused_bn = isinstance(self.bn, BatchNorm2d) and ops.bn_fusable(x, kind, pw, self.bn)
        if fused_bn and training and x.requires_grad and ops.FUSE_SKIP_GRAD:
            # as in the no-norm block: the skip gradient (= the block output gradient, handed over by the second
            # BatchNorm's backward) is added by conv1's data-gradient kernel -- no fan-in pass of its own
            box = ops.GradBox()
            with ops.bn_partial_request():   # the convs leave the BatchNorm's column sums where their kernel can
                c1 = self.conv1.run(x, add_box=box)
            out = self.bn.run(c1, kind, slope, pw)
            with ops.bn_partial_request():
                c2 = self.conv2.run(out)
            return self.bn.run(c2, residual=x, res_box=box)
        if training:
            x, residual = ops.fork(x)  # gradient fan-in summed by srk_axpby
        else:
            residual = x
        if fused_bn:
            # act(bn(conv1)) and bn(conv2) + x each in the BatchNorm's own launches (ONE shared bn: base_networks.py:117)
            with ops.bn_partial_request(training):
                c1 = self.conv1.run(x)
            out = self.bn.run(c1, kind, slope, pw)
            with ops.bn_partial_request(training):
                c2 = self.conv2.run(out)
            return self.bn.run(c2, residual=residual)
        out = self.bn(self.conv1.run(x))
        if self.activation is not None:
            out = self.act(out)
        out = self.bn(self.conv2.run(out))
        return ops.add(out, residual)


class ChannelAttention(torch.nn.Module):
    """The gate of RCAN (Zhang et al. 2018, eq. 4-5): y = t * sigmoid(W_U relu(W_D mean_hw(t))) [+ residual], with the
    official module's parameter names: conv_du.0 = W_D [C/r, C, 1, 1], conv_du.2 = W_U [C, C/r, 1, 1].  One fused op
    (ops.channel_attention), the skip add of the surrounding block included."""

    def __init__(self, num_filter, reduction=16):
        super(ChannelAttention, self).__init__()
        if reduction < 1 or num_filter % reduction != 0:
            raise ValueError("ChannelAttention: %d channels are not divisible by reduction %d" % (num_filter, reduction))
        self.conv_du = torch.nn.Sequential(GateConv2d(num_filter, num_filter // reduction), ReLU(True),
                                           GateConv2d(num_filter // reduction, num_filter), Sigmoid())

    def forward(self, t, residual=None, res_box=None):
        down, up = self.conv_du[0], self.conv_du[2]
        return ops.channel_attention(t, residual, down.weight, down.bias, up.weight, up.bias, res_box)


class RCAB(torch.nn.Module):
    """Residual channel attention block: x + CA(conv2(relu(conv1(x)))) in three ops -- conv1 with its ReLU fused, conv2,
    and the gate with the skip add fused.  In training the skip's gradient (= the block output gradient, which the gate's
    backward hands over untouched) is added by conv1's data-gradient kernel (ops.GradBox), as in ResnetBlock's no-norm
    path; where the input itself needs no gradient there is no fan-in and the tensor is simply used twice (ops.fork)."""

    def __init__(self, num_filter, reduction=16):
        super(RCAB, self).__init__()
        self.conv1 = Conv2d(num_filter, num_filter, 3, 1, 1)
        self.conv2 = Conv2d(num_filter, num_filter, 3, 1, 1)
        self.ca = ChannelAttention(num_filter, reduction)

    def forward(self, x):
        training = grad_mode(x, *self.parameters())
        box = ops.GradBox() if (training and x.requires_grad and ops.FUSE_SKIP_GRAD) else None
        residual = x
        if training and box is None:
            x, residual = ops.fork(x)
        out = self.conv1.run(x, ACT_RELU, add_box=box)
        return self.ca(self.conv2.run(out), residual, res_box=box)


class ResidualGroup(torch.nn.Module):
    """RCAN's residual group: `num_blocks` RCABs, one 3x3 conv, and the group's skip fused into that conv's store."""

    def __init__(self, num_filter, num_blocks, reduction=16):
        super(ResidualGroup, self).__init__()
        self.blocks = torch.nn.Sequential(*[RCAB(num_filter, reduction) for _ in range(num_blocks)])
        self.conv = ConvBlock(num_filter, num_filter, 3, 1, 1, activation=None, norm=None)

    def forward(self, x):
        if grad_mode(x, *self.parameters()):
            x, skip = ops.fork(x)   # gradient fan-in summed by srk_axpby
        else:
            skip = x
        return self.conv(self.blocks(x), residual=skip)


class RDB(torch.nn.Module):
    """Residual dense block of RDN (Zhang et al., CVPR 2018): C 3x3 convs with ReLU, layer c reading the concatenation of
    the block input and the c - 1 outputs before it, a 1x1 local fusion over all of them, and the block's skip.  (The name
    DenseBlock is the reference's Linear block.)  Parameter names as in the official net: convs.{c}.conv.0.{weight,bias},
    LFF.{weight,bias}.  Nothing is concatenated: ops.residual_dense_blocks runs every conv on channel slices of one
    growth buffer (C + 1 launches); models.RDNNet hands all its blocks to one call, this forward runs a block alone."""

    def __init__(self, G0, G, C):
        super(RDB, self).__init__()
        for name, v in (("G0", G0), ("G", G)):
            if v < 16 or v % 16:
                raise ValueError("RDB: %s = %r is not a positive multiple of 16 (the slice convolutions' channel tile)"
                                 % (name, v))
        if G > 64 or G0 > 64:
            raise ValueError("RDB: G = %r, G0 = %r: a slice convolution writes at most 64 channels" % (G, G0))
        if C < 1:
            raise ValueError("RDB: C = %r layers, at least 1" % (C,))
        self.G0, self.G, self.C = G0, G, C
        self.convs = torch.nn.Sequential(*[_RDBConv(G0 + c * G, G) for c in range(C)])
        self.LFF = SliceConv2d(G0 + C * G, G0, 1)

    def block_params(self):
        """(w_1, b_1, ..., w_C, b_C, w_lff, b_lff) as ops.residual_dense_blocks takes a block."""
        out = []
        for m in self.convs:
            out += [m.conv[0].weight, m.conv[0].bias]
        return tuple(out) + (self.LFF.weight, self.LFF.bias)

    def forward(self, x):
        return ops.residual_dense_blocks(x, [self.block_params()])


class _ResidualDenseBlock5(torch.nn.Module):
    """One of the three dense blocks of an RRDB: conv1..conv4 (growth, LeakyReLU 0.2) and conv5 (back to the trunk width),
    all 3x3.  Parameter holder only -- the arithmetic is ops.rrdb_trunk."""

    def __init__(self, nf, gc):
        super(_ResidualDenseBlock5, self).__init__()
        for c in range(4):
            setattr(self, "conv%d" % (c + 1), SliceConv2d(nf + c * gc, gc, 3))
        self.conv5 = SliceConv2d(nf + 4 * gc, nf, 3)

    def block_params(self):
        out = []
        for c in range(5):
            m = getattr(self, "conv%d" % (c + 1))
            out += [m.weight, m.bias]
        return tuple(out)

    def forward(self, x):
        raise RuntimeError("a dense block of an RRDB runs inside ops.rrdb_trunk (base_networks.RRDB.forward)")


class RRDB(torch.nn.Module):
    """Residual-in-residual dense block of ESRGAN (Wang et al., ECCV-W 2018): three dense blocks of five 3x3 convs, each
    v = res_scale * conv5(dense(u)) + u, and the outer out = res_scale * v3 + x.  Parameter names as in BasicSR's
    RRDBNet: rdb{1,2,3}.conv{1..5}.{weight,bias}.  Nothing is concatenated and no scaling or addition is a launch of its
    own: ops.rrdb_trunk runs the 15 convs on channel slices with the scales and both skips in the conv5 epilogues;
    models.RRDBNet hands all its blocks to one call, this forward runs a block alone."""

    def __init__(self, nf, gc=32, res_scale=0.2):
        super(RRDB, self).__init__()
        for name, v in (("nf", nf), ("gc", gc)):
            if v < 16 or v % 16:
                raise ValueError("RRDB: %s = %r is not a positive multiple of 16 (the slice convolutions' channel tile)"
                                 % (name, v))
            if v > 64:
                raise ValueError("RRDB: %s = %r: a slice convolution writes at most 64 channels" % (name, v))
        self.nf, self.gc, self.res_scale = nf, gc, float(res_scale)
        self.rdb1 = _ResidualDenseBlock5(nf, gc)
        self.rdb2 = _ResidualDenseBlock5(nf, gc)
        self.rdb3 = _ResidualDenseBlock5(nf, gc)

    def block_params(self):
        """The three dense blocks' (w1, b1, ..., w5, b5), as ops.rrdb_trunk takes an RRDB."""
        return (self.rdb1.block_params(), self.rdb2.block_params(), self.rdb3.block_params())

    def forward(self, x):
        return ops.rrdb_trunk(x, [self.block_params()], self.res_scale)


class _RDBConv(torch.nn.Module):
    """One growth layer of an RDB; `conv` = Sequential(conv 3x3, ReLU) as in the official net, hence the key conv.0."""

    def __init__(self, in_channels, G):
        super(_RDBConv, self).__init__()
        self.conv = torch.nn.Sequential(SliceConv2d(in_channels, G, 3), ReLU())

    def forward(self, x):
        raise RuntimeError("an RDB layer runs inside ops.residual_dense_blocks (base_networks.RDB.forward)")


class WindowAttention(torch.nn.Module):
    """Window multi-head self-attention with a relative position bias (Swin's W-MSA / SW-MSA), upstream's parameter names:
    `relative_position_bias_table` [(2w - 1)^2, heads], `qkv` and `proj` with nn.Linear's [out, in] weights.  The two
    projections are 1x1 convolutions of the NHWC map (layers.TokenLinear); everything between them -- shift, partition,
    head split, bias gather, mask, softmax and the way back -- is ops.window_attention.  Upstream's
    `relative_position_index` buffer does not exist here: the kernel computes the index."""

    def __init__(self, dim, window_size, num_heads):
        super(WindowAttention, self).__init__()
        ops.window_attention_check(dim, num_heads, window_size, 0, who="WindowAttention")
        self.dim, self.window_size, self.num_heads = dim, int(window_size), int(num_heads)
        self.relative_position_bias_table = torch.nn.Parameter(torch.zeros((2 * self.window_size - 1) ** 2, num_heads))
        torch.nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self.qkv = TokenLinear(dim, dim * 3)
        self.proj = TokenLinear(dim, dim)

    def forward(self, x, shift=0, residual=None):
        """x: logical [N, C, H, W] channels_last; `residual` is added in proj's epilogue."""
        qkv = ops.to_nhwc(self.qkv.run(x)).permute(0, 2, 3, 1)          # [N, H, W, 3C], the storage as it is
        out = ops.window_attention(qkv, self.relative_position_bias_table, self.num_heads, self.window_size, shift)
        return self.proj.run(out.permute(0, 3, 1, 2), residual=residual)


class Mlp(torch.nn.Module):
    """fc1, exact GELU, fc2 per token (upstream's names); `residual` is added in fc2's epilogue."""

    def __init__(self, in_features, hidden_features):
        super(Mlp, self).__init__()
        self.fc1 = TokenLinear(in_features, hidden_features)
        self.act = GELU()
        self.fc2 = TokenLinear(hidden_features, in_features)

    def forward(self, x, residual=None):
        return self.fc2.run(self.act(self.fc1.run(x)), residual=residual)


class SwinTransformerLayer(torch.nn.Module):
    """x + attn(norm1(x)), then x + mlp(norm2(x)) (upstream's SwinTransformerBlock without stochastic depth): eight
    launches, both skips in the epilogues of proj and fc2.  In training each skip's gradient fan-in is one srk_axpby
    (ops.fork)."""

    def __init__(self, dim, num_heads, window_size=8, shift_size=0, mlp_ratio=2.):
        super(SwinTransformerLayer, self).__init__()
        ops.window_attention_check(dim, num_heads, window_size, shift_size, who="SwinTransformerLayer")
        self.shift_size = int(shift_size)
        self.norm1 = LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size, num_heads)
        self.norm2 = LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, x):
        training = grad_mode(x, *self.parameters())
        x, skip = ops.fork(x) if training else (x, x)
        x = self.attn(self.norm1(x), self.shift_size, residual=skip)
        x, skip = ops.fork(x) if training else (x, x)
        return self.mlp(self.norm2(x), residual=skip)


class _SwinLayers(torch.nn.Module):
    """The `residual_group` of an RSTB (upstream's BasicLayer): `blocks`, even ones unshifted, odd ones shifted by half a
    window."""

    def __init__(self, dim, depth, num_heads, window_size, mlp_ratio):
        super(_SwinLayers, self).__init__()
        self.blocks = torch.nn.ModuleList([
            SwinTransformerLayer(dim, num_heads, window_size, 0 if j % 2 == 0 else window_size // 2, mlp_ratio)
            for j in range(depth)])

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return x


class RSTB(torch.nn.Module):
    """Residual Swin Transformer block: `depth` layers, a 3x3 conv, the skip (fused into that conv's store)."""

    def __init__(self, dim, depth, num_heads, window_size=8, mlp_ratio=2.):
        super(RSTB, self).__init__()
        if depth < 1:
            raise ValueError("RSTB: depth %r, at least 1 layer" % (depth,))
        self.residual_group = _SwinLayers(dim, depth, num_heads, window_size, mlp_ratio)
        self.conv = Conv2d(dim, dim, 3, 1, 1)

    def forward(self, x):
        if grad_mode(x, *self.parameters()):
            x, skip = ops.fork(x)   # gradient fan-in summed by srk_axpby
        else:
            skip = x
        return self.conv.run(self.residual_group(x), residual=skip)


class PSBlock(_Block):
    """base_networks.py:153-185 — conv -> PixelShuffle -> [bn] -> [act]; the shuffle is fused into
    the conv's store (the BN, when present, has `output_size` channels and runs after it)."""

    def __init__(self, input_size, output_size, scale_factor, kernel_size=3, stride=1, padding=1, bias=True,
                 activation='relu', norm='batch'):
        super(PSBlock, self).__init__()
        self.conv = Conv2d(input_size, output_size * scale_factor ** 2, kernel_size, stride, padding, bias=bias)
        self.ps = PixelShuffle(scale_factor)
        self._r = int(scale_factor)
        self.conv._ps_r = self._r  # PackPlan packs this conv's filter in pixel-shuffle channel order
        self._setup(output_size, activation, norm)

    def forward(self, x):
        kind, slope, pw = self._act_args()
        training = grad_mode(x, self.conv.weight, self.conv.bias, pw)
        fuse = self.norm is None and (kind == ACT_NONE or not training)
        out = self.conv.run(x, kind if fuse else ACT_NONE, slope, pw if fuse else None, None, self._r)
        return self._post(out, fuse)


class UpsampleNearest(torch.nn.Upsample):
    """torch.nn.Upsample(scale_factor=r, mode='nearest') surface (base_networks.py:206) on srk_upsample_nearest_*."""

    def __init__(self, scale_factor):
        super(UpsampleNearest, self).__init__(scale_factor=scale_factor, mode='nearest')
        self._r = int(scale_factor)

    def forward(self, x):
        return ops.upsample_nearest(x, self._r)


class Upsample2xBlock(torch.nn.Module):
    """base_networks.py:188-214"""

    def __init__(self, input_size, output_size, bias=True, upsample='deconv', activation='relu', norm='batch'):
        super(Upsample2xBlock, self).__init__()
        scale_factor = 2
        if upsample == 'deconv':
            self.upsample = DeconvBlock(input_size, output_size, kernel_size=4, stride=2, padding=1, bias=bias,
                                        activation=activation, norm=norm)
        elif upsample == 'ps':
            self.upsample = PSBlock(input_size, output_size, scale_factor=scale_factor, bias=bias,
                                    activation=activation, norm=norm)
        elif upsample == 'rnc':
            # 3. Resize and Convolution (base_networks.py:204-210): nn.Sequential(Upsample(x2, nearest), ConvBlock 3x3)
            # — same container and indices, so the state_dict keys are `upsample.1.conv.weight` etc. like the reference
            self.upsample = torch.nn.Sequential(
                UpsampleNearest(scale_factor),
                ConvBlock(input_size, output_size, kernel_size=3, stride=1, padding=1, bias=bias,
                          activation=activation, norm=norm))
        else:
            raise ValueError("unknown upsample mode %r" % (upsample,))

    def forward(self, x):
        return self.upsample(x)
