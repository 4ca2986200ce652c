"""Tiled super-resolution of pictures too large (or too thin a batch) for one pass: geometry of the nets and the tile plan.

Host only, exact integer arithmetic, importable without a GPU.  The device side is csrc/tile.hip (ops.tile_gather /
tile_stitch / tile_stitch_u8); the trainers drive both from sr_trainers._Trainer._infer_tiled.

The reference's eight nets are convolutional with a bounded receptive field and treat both axes alike, so everything
here is one-dimensional and applied to rows and columns independently.  The ninth, RCAN, is not: its channel attention
pools over the whole picture, the walk says so (as it does for instance norm) and the picture runs in one pass.  The
tenth, RDN, is convolutional again: a residual dense block is the cone of its C chained 3x3 convs.  The eleventh, SwinIR,
cuts the whole picture into windows and masks by its borders: refused like RCAN.

Geometry.  Along one axis, a feature map of a net is described against the net's INPUT by three integers (scale, lo, hi):
map pixel o depends on the input pixels

    floor((o + lo) / scale) .. floor((o + hi) / scale)                        (the unclipped cone; lo <= 0 <= hi here)

clipped to the picture, and a map of an input of n pixels has scale * n + offset pixels.  The layers compose exactly:

    conv k, stride 1, pad p      lo -= p                    hi += k - 1 - p            offset += 2p - k + 1
    PixelShuffle / nearest x r   lo *= r                    hi *= r                    scale *= r, offset *= r
    deconv k, stride t, pad p    lo = lo * t + p - k + t    hi = hi * t + p            scale *= t,
                                                                     offset = (offset - 1) * t - 2p + k + output_padding
    a + b (skip, pyramid sum)    lo = min, hi = max         (both operands have one scale and one offset)

(floor(floor(o / r) + a) / s) = floor((o + a r) / (s r)) for integers, which is why one pair of integers survives an
up-sampler.)  Activations and eval-mode BatchNorm are pointwise.  Clipping once, at the input, equals clipping at every
layer because every map of these nets covers the whole input: tests/test_tile_cpu.py checks the derived cones against
the NaN support of the reference nets, in both directions.

net_geometry() derives the triple by walking the module objects in the order the net's forward composes them, reading
kernel size, stride, padding, up-sampling factor, block counts and recursion count from the modules themselves.

Plan.  Tiles have one size, min(tile, extent) per axis, and lie inside the picture; the last one is shifted inwards.  A
tile at input offset x computes output pixel o = q + scale * x at its local position q, and computes it RIGHT iff the
clipped cone of o lies inside [x, x + T): where the unclipped cone leaves the tile, the tile's edge is then the
picture's edge and the net's zero padding there is the one-pass padding.  That is an interval of o per tile; the step
between tiles is the largest for which consecutive intervals abut, and every output pixel is owned by the FIRST tile
whose interval holds it.

Self-ensemble.  The x8 ensemble (sr_trainers: self_ensemble) also runs the net on mirrored and rotated pictures and maps
the results back.  Both axes are alike, so a rotation only swaps which axis a cone applies to; what changes a cone is
the mirror.  With J the reversal of an axis of n input pixels (i -> n - 1 - i) and J' that of its N = scale n + offset
output pixels, the mirrored net is x -> J' f(J x), and its output pixel o depends on J(cone of N - 1 - o):

    n - 1 - floor((N - 1 - o + hi) / s) .. n - 1 - floor((N - 1 - o + lo) / s)

and with N = s n + offset and -floor(-a / s) - 1 = floor((a - 1) / s) that is

    floor((o - offset - hi) / s) .. floor((o - offset - lo) / s)

so mirrored(g) = Geometry(scale, offset, -offset - hi, -offset - lo): the extent n has cancelled, hence one geometry
serves the picture and every tile.  A cone with lo + hi = -offset is its own mirror image (every net here except FSRCNN,
whose transposed conv makes it lopsided: x4 (-18, 35) against (-19, 34)).  The ensemble of a tile is right at an output
pixel iff the tile is right there for the net AND for the mirrored net, so the plan of an ensemble run comes from
ensemble_geometry(g), the union of the two cones.
"""
from fractions import Fraction

import torch

# tile='auto': one pass while the widest per-image activation of the picture stays under AUTO_BUDGET_BYTES, else tiles of
# AUTO_TILE net-input pixels in chunks of DEFAULT_TILE_BATCH tiles.  From the sweep of DESIGN.md 17 (profiles/tile_*.txt):
# one pass is faster than every tiling wherever it runs on the fast conv kernels, so the budget is their limit itself, a
# per-image activation of 2^31 bytes (32-bit byte offsets in their buffer descriptors); among tilings the largest tile
# measured wins (least overlap recomputed), and at that size the chunk length moves the time by under 5 %, so the chunk is
# the shortest measured: its working set is the smallest.
AUTO_BUDGET_BYTES = (1 << 31) - 1
AUTO_TILE = 384
DEFAULT_TILE_BATCH = 4


class Geometry(object):
    """One axis of a net's output against its input (see the module text).  `floats_per_pixel` is the widest activation
    of the net in fp32 values per input pixel (channels * scale^2 of the largest map), for the 'auto' budget."""

    __slots__ = ("scale", "offset", "lo", "hi", "floats_per_pixel")

    def __init__(self, scale=1, offset=0, lo=0, hi=0, floats_per_pixel=0):
        self.scale, self.offset, self.lo, self.hi, self.floats_per_pixel = scale, offset, lo, hi, floats_per_pixel

    def out_size(self, n):
        return self.scale * n + self.offset

    def span(self, o):
        """(first, last) input pixel of the unclipped dependency cone of output pixel o."""
        return (o + self.lo) // self.scale, (o + self.hi) // self.scale

    def clipped_span(self, o, n):
        a, b = self.span(o)
        return max(a, 0), min(b, n - 1)

    @property
    def origin(self):
        """Centre of the cone of output pixel o, in input pixels, is o / scale + origin."""
        return Fraction(self.lo + self.hi, 2 * self.scale)

    @property
    def reach(self):
        """Half-width of the cone in input pixels: o / scale + origin +- reach bounds the input pixels o depends on."""
        return Fraction(self.hi - self.lo, 2 * self.scale)

    @property
    def min_tile(self):
        """Smallest tile (input pixels) with which tiling advances at all: step = floor(T - (hi - lo) / scale) >= 1."""
        return -(-(self.hi - self.lo + self.scale) // self.scale)

    def __repr__(self):
        return "Geometry(scale=%d, offset=%d, lo=%d, hi=%d; origin %s, reach %s)" % (
            self.scale, self.offset, self.lo, self.hi, self.origin, self.reach)


# ---- the walk ------------------------------------------------------------------------------------------------------------
def _one(v, what, path):
    v = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if v[0] != v[1]:
        raise ValueError("%s: anisotropic %s %r has no tiling geometry" % (path, what, v))
    return int(v[0])


def _conv(g, m, path):
    k, s, p = _one(m.kernel_size, "kernel", path), _one(m.stride, "stride", path), _one(m.padding, "padding", path)
    if s != 1 or _one(m.dilation, "dilation", path) != 1:
        raise ValueError("%s: a conv of stride %d / dilation %r has no tiling geometry" % (path, s, m.dilation))
    return Geometry(g.scale, g.offset + 2 * p - k + 1, g.lo - p, g.hi + k - 1 - p,
                    max(g.floats_per_pixel, m.out_channels * g.scale ** 2))


def _deconv(g, m, path):
    k, t, p = _one(m.kernel_size, "kernel", path), _one(m.stride, "stride", path), _one(m.padding, "padding", path)
    op = _one(m.output_padding, "output_padding", path)
    if _one(m.dilation, "dilation", path) != 1:
        raise ValueError("%s: a dilated transposed conv has no tiling geometry" % path)
    # output o takes input i with o = i t - p + j, 0 <= j < k:  ceil((o + p - k + 1) / t) <= i <= floor((o + p) / t)
    return Geometry(g.scale * t, (g.offset - 1) * t - 2 * p + k + op, g.lo * t + p - k + t, g.hi * t + p,
                    max(g.floats_per_pixel, m.out_channels * (g.scale * t) ** 2))


def _upsample(g, r):
    return Geometry(g.scale * r, g.offset * r, g.lo * r, g.hi * r, g.floats_per_pixel)


def _union(a, b, path):
    if a.scale != b.scale or a.offset != b.offset:
        raise ValueError("%s: the operands of a sum have different sizes (%r, %r)" % (path, a, b))
    return Geometry(a.scale, a.offset, min(a.lo, b.lo), max(a.hi, b.hi), max(a.floats_per_pixel, b.floats_per_pixel))


_POINTWISE = (torch.nn.ReLU, torch.nn.LeakyReLU, torch.nn.PReLU, torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Identity)
_WHOLE_IMAGE = (torch.nn.modules.instancenorm._InstanceNorm, torch.nn.GroupNorm, torch.nn.LayerNorm)


def _norm(g, block, path):
    """A block's norm: instance norm and training-mode BatchNorm make every pixel depend on the whole image."""
    bn = getattr(block, "bn", None)
    if getattr(block, "norm", None) == "instance" or isinstance(bn, _WHOLE_IMAGE):
        raise ValueError("%s: norm='instance' depends on the whole image and cannot be tiled" % path)
    if bn is not None:
        return _walk(g, bn, path + ".bn")
    return g


def _walk(g, m, path):
    """Geometry after module m, given geometry g before it."""
    from . import base_networks as B
    if isinstance(m, torch.nn.Sequential):
        for name, child in m.named_children():
            g = _walk(g, child, "%s.%s" % (path, name))
        return g
    if isinstance(m, B.ConvBlock):
        return _norm(_conv(g, m.conv, path + ".conv"), m, path)
    if isinstance(m, B.DeconvBlock):
        return _norm(_deconv(g, m.deconv, path + ".deconv"), m, path)
    if isinstance(m, B.PSBlock):
        return _norm(_upsample(_conv(g, m.conv, path + ".conv"), int(m.ps.upscale_factor)), m, path)
    if isinstance(m, B.ResnetBlock):   # x + bn(conv2(act(bn(conv1(x)))))
        out = _norm(_conv(g, m.conv1, path + ".conv1"), m, path)
        out = _norm(_conv(out, m.conv2, path + ".conv2"), m, path)
        return _union(out, g, path)
    if isinstance(m, B.Upsample2xBlock):
        return _walk(g, m.upsample, path + ".upsample")
    if isinstance(m, B.ChannelAttention):   # its gate is a function of every pixel of the picture
        raise ValueError("%s: ChannelAttention depends on the whole image and cannot be tiled" % path)
    if isinstance(m, B.WindowAttention):   # the window grid and the border mask belong to the whole picture
        raise ValueError("%s: WindowAttention partitions the whole image into windows and cannot be tiled" % path)
    if isinstance(m, B.SwinTransformerLayer):
        return _union(_walk(g, m.attn, path + ".attn"), g, path)
    if isinstance(m, B.RSTB):
        out = g
        for name, blk in m.residual_group.blocks.named_children():
            out = _walk(out, blk, "%s.residual_group.blocks.%s" % (path, name))
        return _union(_walk(out, m.conv, path + ".conv"), g, path)
    if isinstance(m, B.RCAB):   # x + ca(conv2(relu(conv1(x))))
        out = _conv(_conv(g, m.conv1, path + ".conv1"), m.conv2, path + ".conv2")
        return _union(_walk(out, m.ca, path + ".ca"), g, path)
    if isinstance(m, B.ResidualGroup):
        return _union(_walk(_walk(g, m.blocks, path + ".blocks"), m.conv, path + ".conv"), g, path)
    if isinstance(m, B.RDB):   # x + LFF(cat(x, y_1 .. y_C)), y_c = relu(conv_c(cat(x, y_1 .. y_c-1))): the deepest cone is
        out = g                # the chain of all C 3x3 convs, the 1x1 fusion adds nothing, the skip is the input itself
        for name, layer in m.convs.named_children():
            out = _union(_conv(out, layer.conv[0], "%s.convs.%s.conv.0" % (path, name)), g, path)
        out = _union(_conv(out, m.LFF, path + ".LFF"), g, path)
        # live while the block runs: its input, the growth buffer and its output
        live = (2 * m.G0 + m.C * m.G) * g.scale ** 2
        return Geometry(out.scale, out.offset, out.lo, out.hi, max(out.floats_per_pixel, live))
    if isinstance(m, B.RRDB):   # 15 chained 3x3 convs a block: 23 blocks reach about 350 input pixels to each side
        raise ValueError("%s: RRDB: the trunk's dependency cone (15 pixels a block to each side) leaves a tile mostly halo; "
                         "ESRGAN's pictures run in one pass" % path)
    if isinstance(m, torch.nn.ConvTranspose2d):
        return _deconv(g, m, path)
    if isinstance(m, torch.nn.Conv2d):
        return _conv(g, m, path)
    if isinstance(m, torch.nn.PixelShuffle):
        return _upsample(g, int(m.upscale_factor))
    if isinstance(m, torch.nn.Upsample):
        r = m.scale_factor
        if m.mode != "nearest" or r is None or int(r) != r:
            raise ValueError("%s: only integer nearest-neighbour up-sampling has a tiling geometry" % path)
        return _upsample(g, int(r))
    if isinstance(m, _models().MotionCompensator):
        raise ValueError("%s: MotionCompensator warps by a learned flow, its reach depends on the picture and cannot be "
                         "tiled" % path)
    if isinstance(m, _WHOLE_IMAGE):
        raise ValueError("%s: %s depends on the whole image and cannot be tiled" % (path, type(m).__name__))
    if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
        if m.training or m.running_mean is None:
            raise ValueError("%s: BatchNorm in training mode (batch statistics) depends on the whole image and cannot be "
                             "tiled; call model.eval() first" % path)
        return g
    if isinstance(m, _POINTWISE):
        return g
    raise ValueError("%s: no tiling geometry for a %s" % (path, type(m).__name__))


def _models():
    from . import models
    return models


def net_geometry(model):
    """Geometry of one of the package's nets, derived from its modules: the composition follows each net's forward
    (models.py), every number comes from the module objects.  Raises ValueError for a module whose result depends on the
    whole image (it names the module) and for a net it does not know how to compose."""
    from . import models as M
    g = Geometry()
    if isinstance(model, (M.SRCNNNet, M.ESPCNNet)):
        return _walk(g, model.layers, "layers")
    if isinstance(model, M.FSRCNNNet):
        g = _walk(g, model.first_part, "first_part")
        g = _walk(g, model.mid_part, "mid_part")
        return _walk(g, model.last_part, "last_part")
    if isinstance(model, M.VDSRNet):
        out = _walk(_walk(g, model.input_conv, "input_conv"), model.residual_layers, "residual_layers")
        return _union(_walk(out, model.output_conv, "output_conv"), g, "output_conv")
    if isinstance(model, (M.EDSRNet, M.SRGANGenerator)):
        head = _walk(g, model.input_conv, "input_conv")
        out = _walk(_walk(head, model.residual_layers, "residual_layers"), model.mid_conv, "mid_conv")
        out = _union(out, head, "mid_conv")
        return _walk(_walk(out, model.upscale4x, "upscale4x"), model.output_conv, "output_conv")
    if isinstance(model, M.RCANNet):   # raises at the first channel attention; the composition is the forward's all the same
        head = _walk(g, model.input_conv, "input_conv")
        out = _walk(_walk(head, model.residual_groups, "residual_groups"), model.mid_conv, "mid_conv")
        out = _union(out, head, "mid_conv")
        return _walk(_walk(out, model.upscale, "upscale"), model.output_conv, "output_conv")
    if isinstance(model, M.SwinIRNet):   # raises at the first window attention
        head = _walk(g, model.conv_first, "conv_first")
        out = head
        for name, layer in model.layers.named_children():
            out = _walk(out, layer, "layers.%s" % name)
        return out
    if isinstance(model, M.RDNNet):
        head = _walk(g, model.SFENet1, "SFENet1")
        out = _walk(head, model.SFENet2, "SFENet2")
        fused = None   # the fusion buffer: every block's output, block d + 1 reading block d's
        for name, block in model.RDBs.named_children():
            out = _walk(out, block, "RDBs.%s" % name)
            fused = out if fused is None else _union(fused, out, "RDBs.%s" % name)
        rdb = model.RDBs[0]
        # live through the trunk: the SFENet1 skip, the trunk's input, the whole fusion buffer and one growth buffer
        live = (2 * rdb.G0 + len(model.RDBs) * rdb.G0 + rdb.C * rdb.G) * fused.scale ** 2
        fused = Geometry(fused.scale, fused.offset, fused.lo, fused.hi, max(fused.floats_per_pixel, live))
        out = _union(_walk(fused, model.GFF, "GFF"), head, "GFF")
        return _walk(out, model.UPNet, "UPNet")
    if isinstance(model, M.RRDBNet):   # raises at the first RRDB
        return _walk(_walk(g, model.conv_first, "conv_first"), model.body[0], "body.0")
    if isinstance(model, M.LapSRNNet):
        f1 = _walk(_walk(g, model.input_conv, "input_conv"), model.convt_F1, "convt_F1")
        coarse = _union(_walk(f1, model.convt_R1, "convt_R1"), _walk(g, model.convt_I1, "convt_I1"), "convt_R1")
        f2 = _walk(f1, model.convt_F2, "convt_F2")
        return _union(_walk(f2, model.convt_R2, "convt_R2"), _walk(coarse, model.convt_I2, "convt_I2"), "convt_R2")
    if isinstance(model, M.DRCNNet):
        h = _walk(g, model.embedding_layer, "embedding_layer")
        out = g   # x + sum_d w_d * reconstruction(h_d)
        for _ in range(int(model.num_recursions)):
            h = _walk(h, model.conv_block, "conv_block")
            out = _union(out, _walk(h, model.reconstruction_layer, "reconstruction_layer"), "reconstruction_layer")
        return out
    if isinstance(model, M.VESPCNNet):   # raises at the MotionCompensator
        return _walk(_walk(g, model.mc, "mc"), model.layers, "layers")
    raise ValueError("net_geometry: no composition rule for a %s" % type(model).__name__)


def mirrored(g):
    """Geometry of the net wrapped in a reversal of the axis, before and after (the module text has the derivation)."""
    return Geometry(g.scale, g.offset, -g.offset - g.hi, -g.offset - g.lo, g.floats_per_pixel)


def ensemble_geometry(g):
    """Geometry under which a tile is right for all eight variants of the self-ensemble: the union of both cones."""
    return _union(g, mirrored(g), "self-ensemble")


# ---- the plan ------------------------------------------------------------------------------------------------------------
class AxisPlan(object):
    """Tiles of one axis: `starts` (input offset of each tile) and `own` ([first, end) output pixels each tile owns)."""

    def __init__(self, g, n, tile):
        self.n, self.tile = n, min(tile, n)
        self.n_out, self.tile_out = g.out_size(n), g.out_size(self.tile)
        T, s = self.tile, g.scale
        if self.n_out < 1:
            raise ValueError("an extent of %d input pixels is smaller than the net's border (%d)" % (n, 1 - g.offset))
        if T == n:
            self.starts, self.own = [0], [(0, self.n_out)]
            return
        step = (s * T - (g.hi - g.lo)) // s
        if step < 1:
            raise ValueError("tile=%d is too small for this net: its dependency cone spans %s input pixels, the minimum "
                             "tile is %d" % (tile, 2 * g.reach, g.min_tile))
        count = -(-(n - T) // step) + 1
        self.starts = [min(j * step, n - T) for j in range(count)]
        self.own, first = [], 0
        for j, x in enumerate(self.starts):
            # the last output pixel whose cone ends inside this tile: floor((o + hi) / s) <= x + T - 1
            end = self.n_out if j == count - 1 else min(s * (x + T) - g.hi, s * x + self.tile_out)
            # (the first it may own is the first whose cone starts inside it: o >= s x - lo; the step guarantees it)
            if not first < end or (j > 0 and first < s * x - g.lo):
                raise AssertionError("no exact ownership for tile %d of %r under %r" % (j, self.starts, g))
            self.own.append((first, end))
            first = end

    def __len__(self):
        return len(self.starts)


class Plan(object):
    """Equal tiles of a picture of H x W net-input pixels (rows x cols, tile t = row * len(cols) + col)."""

    def __init__(self, g, H, W, tile):
        self.geometry, self.H, self.W = g, int(H), int(W)
        self.rows, self.cols = AxisPlan(g, self.H, tile), AxisPlan(g, self.W, tile)
        self.th, self.tw = self.rows.tile, self.cols.tile
        self.oth, self.otw = self.rows.tile_out, self.cols.tile_out
        self.OH, self.OW = self.rows.n_out, self.cols.n_out
        self.ntiles = len(self.rows) * len(self.cols)

    def tiles(self):
        """(t, (y0, x0) input corner, ((oy0, oy1), (ox0, ox1)) owned output rectangle), in plan order."""
        t = 0
        for y0, oy in zip(self.rows.starts, self.rows.own):
            for x0, ox in zip(self.cols.starts, self.cols.own):
                yield t, (y0, x0), (oy, ox)
                t += 1

    def table(self):
        """The device table: int32 [len(rows) + len(cols)][4], rows first; an entry is (input offset, first owned output
        pixel, end of the owned output pixels, output pixel of the tile's local pixel 0 = scale * input offset)."""
        s = self.geometry.scale
        return [[x, o[0], o[1], s * x] for ax in (self.rows, self.cols) for x, o in zip(ax.starts, ax.own)]


def plan(geometry, H, W, tile):
    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be a positive number of net-input pixels, got %d" % tile)
    return Plan(geometry, H, W, tile)


def tiles_per_chunk(tile_batch, ntiles, ensemble=False):
    """Tiles per batch of the tiled loop from the `tile_batch` option (None: DEFAULT_TILE_BATCH; 'all' / 0: every tile).
    With the self-ensemble a tile is eight net inputs and `tile_batch` counts net inputs, rounded up to whole tiles, so a
    given tile_batch means the same working set with and without it."""
    if tile_batch in ('all', 0):
        return max(1, int(ntiles))
    n = max(1, int(DEFAULT_TILE_BATCH if tile_batch is None else tile_batch))
    return -(-n // 8) if ensemble else n


def activation_bytes(geometry, H, W):
    """fp32 bytes of the widest per-image activation of a one-pass run on an H x W net input."""
    return 4 * geometry.floats_per_pixel * int(H) * int(W)


def resolve_tile(tile, geometry, H, W):
    """The `tile` option -> None (one pass) or the tile size: None / 0 / 'none' is off, 'auto' tiles pictures whose widest
    activation exceeds AUTO_BUDGET_BYTES, a number is taken as given."""
    if tile is None or tile == 0 or (isinstance(tile, str) and tile.lower() in ("none", "off", "0")):
        return None
    if isinstance(tile, str) and tile.lower() == "auto":
        return None if activation_bytes(geometry, H, W) <= AUTO_BUDGET_BYTES else AUTO_TILE
    return int(tile)

