"""Case tables and fp64 runners of the configuration matrix (no GPU, no package code in the arithmetic):

  CONFIGS                  every (net, channels, scale, crop) point the command line reaches: product class, oracle class,
                           constructor arguments, input shape, fill gain.  It extends test_nets_gpu.CASES and keeps its seeds
                           (weights 1234, input 4321, output gradients 77 + i scaled by 1 / numel) and its shapes.
  make_oracle / run_oracle the oracle of a configuration (oracle/ref_modules.py, tests/ca_ref.RefRCAN for RCAN) in fp32 or
                           fp64: train-mode outputs, input gradient, every parameter gradient, the buffers after that
                           forward, and the eval-mode outputs that follow.  The fp64 result is computed once and shared.
  bar_* / compare          how much of each bar a tensor uses (1.0 = on the bar); compare() lists every check of a run.
  derive_layer_rows        the conv / transposed-conv / linear layers of all configurations that neither
                           oracle/kat_table.CONV_KATS nor a parametrisation of tests/test_ops_gpu.py already runs.
  LAYER_ROWS               that list, committed as a literal; tests/test_net_configs_cpu.py re-derives it.
  DENSE_EXTRA              dense shapes that reach the branches the real layers do not.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import ca_ref
from oracle import fill, ref_modules as R
from oracle.kat_table import CONV_KATS

TOL_FWD = 1e-4      # max-norm bar of every forward output (tests/test_nets_gpu.py)
RTOL = 1e-3         # element-wise bar of outputs and gradients: the project's contract
SEED_W, SEED_X, SEED_G = 1234, 4321, 77

Config = collections.namedtuple("Config", "name product oracle args ishape gain")


def _configs():
    out = []
    for c in (1, 3):
        out.append(Config("srcnn_c%d" % c, "SRCNNNet", "SRCNN", (c, 64), (2, c, 20, 20), 1.0))
        out.append(Config("vdsr_c%d" % c, "VDSRNet", "VDSR", (c, 64, 18), (2, c, 13, 13), 1.0))
        out.append(Config("edsr_c%d" % c, "EDSRNet", "EDSR", (c, 64, 16), (2, c, 8, 8), 0.5))
        out.append(Config("lapsrn_c%d" % c, "LapSRNNet", "LapSRN", (c, 64, 10), (1, c, 8, 8), 1.0))
        out.append(Config("srgan_g_c%d" % c, "SRGANGenerator", "Generator", (c, 64, 16), (2, c, 8, 8), 0.7))
    for c in (1, 3):
        for r in (2, 3, 4, 8):
            out.append(Config("espcn_c%d_x%d" % (c, r), "ESPCNNet", "ESPCN", (c, 64, r), (2, c, 16, 16), 1.0))
    for c in (1, 3):
        for r in (2, 3, 4):
            out.append(Config("fsrcnn_c%d_x%d" % (c, r), "FSRCNNNet", "FSRCNN", (c, r, 56, 12, 4), (2, c, 12, 12), 1.0))
    for c in (1, 3):
        for r in (2, 4, 8):
            out.append(Config("rcan_c%d_x%d" % (c, r), "RCANNet", "RefRCAN", (c, 64, 1, 2, 16, r), (2, c, 9, 11), 0.5))
    for c in (1, 3):
        for crop in (16, 32, 48, 96):
            out.append(Config("srgan_d_c%d_crop%d" % (c, crop), "SRGANDiscriminator", "Discriminator", (c, 64, crop),
                              (3, c, crop, crop), 1.0))
    return collections.OrderedDict((c.name, c) for c in out)


CONFIGS = _configs()
NET_CONFIGS = [n for n in CONFIGS if not n.startswith("srgan_d")]      # forward and every gradient
DISC_CONFIGS = [n for n in CONFIGS if n.startswith("srgan_d")]         # forward and running statistics only


def oracle_class(cfg):
    return ca_ref.RefRCAN if cfg.oracle == "RefRCAN" else getattr(R, cfg.oracle)


def make_oracle(cfg):
    """The configuration's oracle in fp32 with the seeded weights; its state_dict is what the product net loads."""
    return fill.fill_module(oracle_class(cfg)(*cfg.args), SEED_W, cfg.gain)


def _as_list(y):
    return list(y) if isinstance(y, (tuple, list)) else [y]


def out_grads(outs):
    return [fill.randn(tuple(y.shape), SEED_G + i) / y.numel() for i, y in enumerate(outs)]


Ref = collections.namedtuple("Ref", "outs dx grads buffers eval_outs")


def _run(name, dtype, backward):
    cfg = CONFIGS[name]
    ora = make_oracle(cfg).to(dtype).train()
    x = fill.rand(cfg.ishape, SEED_X).to(dtype).requires_grad_(backward)
    outs = _as_list(ora(x))
    dx, grads = None, {}
    if backward:
        torch.autograd.backward(outs, [g.to(dtype) for g in out_grads(outs)])
        dx = x.grad.detach()
        grads = collections.OrderedDict((k, p.grad.detach()) for k, p in ora.named_parameters())
    buffers = collections.OrderedDict((k, b.detach().clone()) for k, b in ora.named_buffers())
    ora.eval()
    with torch.no_grad():
        eval_outs = _as_list(ora(x.detach()))
    return Ref([y.detach() for y in outs], dx, grads, buffers, eval_outs)


@functools.lru_cache(maxsize=None)
def run_oracle(name, backward=True):
    """The fp64 reference of a configuration, computed once and left unchanged."""
    return _run(name, torch.float64, backward)


def run_oracle_fp32(name, backward=True):
    return _run(name, torch.float32, backward)


# ---- how much of a bar a tensor uses ------------------------------------------------------------------------------------
def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().double().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def bar_maxnorm(a, b, tol):
    """conftest.rel_err(a, b) / tol."""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30) / tol


def bar_elementwise(a, b, rtol):
    """max over elements of |a - b| / (atol + rtol |b|) with conftest.assert_close_elementwise's atol = rtol * rms(b)."""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if not b.size:
        return 0.0
    atol = rtol * float(np.sqrt(np.mean(b * b)))
    den = atol + rtol * np.abs(b)
    err = np.abs(a - b)
    if not err.any():
        return 0.0
    return float((err / np.maximum(den, 1e-300)).max())


def compare(name, got, ref):
    """Every check of one run as (what, bar, share of the bar used): outputs element-wise at RTOL and max-norm at TOL_FWD,
    dx and every parameter gradient element-wise at RTOL (a gradient that is mathematically zero -- the bias of a conv in
    front of a BatchNorm, |ref| < 1e-6 of the largest gradient rms -- must be noise-sized: below 1e-5 of that scale, the rule
    of test_net_elementwise_outputs_and_body_gradients), float buffers like outputs, eval outputs max-norm at TOL_FWD."""
    rows = []
    for i, (a, b) in enumerate(zip(got.outs, ref.outs)):
        rows.append(("%s output %d" % (name, i), "elementwise 1e-3", bar_elementwise(a, b, RTOL)))
        rows.append(("%s output %d" % (name, i), "max-norm 1e-4", bar_maxnorm(a, b, TOL_FWD)))
    assert len(got.outs) == len(ref.outs)
    if ref.dx is not None:
        rows.append((name + " dx", "elementwise 1e-3", bar_elementwise(got.dx, ref.dx, RTOL)))
        gscale = max(float(g.double().pow(2).mean().sqrt()) for g in ref.grads.values())
        assert list(got.grads) == list(ref.grads)
        for k, b in ref.grads.items():
            a = got.grads[k]
            if float(b.abs().max()) < 1e-6 * gscale:
                rows.append(("%s grad %s" % (name, k), "zero: max < 1e-5 scale", float(a.abs().max()) / (1e-5 * gscale)))
            else:
                rows.append(("%s grad %s" % (name, k), "elementwise 1e-3", bar_elementwise(a, b, RTOL)))
    for k, b in ref.buffers.items():
        a = got.buffers[k]
        if not torch.is_floating_point(b):
            assert int(a) == int(b), (name, k, int(a), int(b))
            continue
        rows.append(("%s buffer %s" % (name, k), "elementwise 1e-3", bar_elementwise(a, b, RTOL)))
        rows.append(("%s buffer %s" % (name, k), "max-norm 1e-4", bar_maxnorm(a, b, TOL_FWD)))
    for i, (a, b) in enumerate(zip(got.eval_outs, ref.eval_outs)):
        rows.append(("%s eval output %d" % (name, i), "max-norm 1e-4", bar_maxnorm(a, b, TOL_FWD)))
    return rows


def worst(rows):
    return max(rows, key=lambda r: r[2])


# ---- the layers these configurations add --------------------------------------------------------------------------------
# key: (kind, Cin, Cout, k, stride, pad, output_padding, act, ps_r); kind is "conv", "deconv" or "linear" (k = stride = 0)
def _layer_act(parent, leaf):
    """The activation that directly follows the layer (fused into its epilogue by the package): none when a norm sits in
    between, none behind the second conv of a residual block."""
    if isinstance(parent, R.ResnetBlock):
        return parent.activation if (leaf == "conv1" and parent.norm is None) else None
    if isinstance(parent, R._Blk):
        return parent.activation if parent.norm is None else None
    if isinstance(parent, ca_ref._RCAB):
        return "relu" if leaf == "conv1" else None
    return None


def oracle_layer_keys(model):
    """Walk an oracle: its conv, transposed-conv and linear modules with what follows them (the channel-attention gates'
    1x1 convs are part of the gate operator, not conv layers: tests/test_ca_gpu.py)."""
    mods = dict(model.named_modules())
    keys = []
    for name, m in mods.items():
        if ".conv_du." in "." + name or not isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
            continue
        parent_name, _, leaf = name.rpartition(".")
        parent = mods[parent_name]
        act = _layer_act(parent, leaf)
        ps = 0
        if isinstance(parent, R.PSBlock):
            ps = parent.ps.upscale_factor
        elif isinstance(parent, ca_ref._Wrapped) and isinstance(mods[parent_name.rpartition(".")[0]], ca_ref._Up):
            ps = 2
        if isinstance(m, nn.Linear):
            keys.append(("linear", m.in_features, m.out_features, 0, 0, 0, 0, act, 0))
        else:
            assert m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1]
            tr = isinstance(m, nn.ConvTranspose2d)
            keys.append(("deconv" if tr else "conv", m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0],
                         m.padding[0], m.output_padding[0] if tr else 0, act, ps))
    return keys


# what the parametrised tests of tests/test_ops_gpu.py apply without naming it in their argument lists
_OPS_IMPLICIT = {
    "test_conv_few_output_channels": {"act": "lrelu"},
    "test_conv_rows_on_n_kernel": {"act": "lrelu"},
    "test_strided_data_gradient_phases_in_one_launch": {"s": 2},
    "test_conv_image_gradient_with_mask": {"act": "lrelu"},
    "test_deconv_large_halo_small_problem": {"tr": 1},
}


def covered_keys():
    """The keys CONV_KATS and the parametrisations of tests/test_ops_gpu.py (those that name cin, cout, k and p) run."""
    import test_ops_gpu as T
    seen = set()
    for tag, cin, cout, k, s, p, tr, op, H, W, N, act in CONV_KATS:
        seen.add(("deconv" if tr else "conv", cin, cout, k, s, p, op, act, 0))
    for fname in sorted(vars(T)):
        fn = getattr(T, fname)
        if not fname.startswith("test_") or not callable(fn):
            continue
        for mark in getattr(fn, "pytestmark", []):
            if mark.name != "parametrize":
                continue
            names = [a.strip() for a in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
            if not {"cin", "cout", "k", "p"} <= set(names):
                continue
            for values in mark.args[1]:
                v = dict(_OPS_IMPLICIT.get(fname, {}))
                v.update(zip(names, getattr(values, "values", values)))
                if "slope" in v:        # a data gradient under the mask of LeakyReLU(slope) / ReLU
                    v["act"] = "lrelu" if v["slope"] else "relu"
                seen.add(("deconv" if v.get("tr") else "conv", v["cin"], v["cout"], v["k"], v.get("s", 1), v["p"],
                          v.get("op", 0), v.get("act"), v.get("ps", 0)))
    return seen


def derive_layer_rows():
    """LAYER_ROWS from scratch: every key of every configuration, in table order, first configuration named, minus
    covered_keys().  The nets are built on the meta device: only their shapes are read."""
    seen = covered_keys()
    rows = []
    for cfg in CONFIGS.values():
        with torch.device("meta"):
            model = oracle_class(cfg)(*cfg.args)
        for key in oracle_layer_keys(model):
            if key not in seen:
                seen.add(key)
                rows.append(key + (cfg.name,))
    return rows


LAYER_ROWS = [
    # (kind, Cin, Cout, k, stride, pad, output_padding, act, ps_r, a configuration it comes from)
    ('conv', 1, 64, 9, 1, 0, 0, 'relu', 0, 'srcnn_c1'),
    ('conv', 64, 32, 5, 1, 0, 0, 'relu', 0, 'srcnn_c1'),
    ('conv', 32, 1, 5, 1, 0, 0, None, 0, 'srcnn_c1'),
    ('conv', 1, 64, 3, 1, 1, 0, 'relu', 0, 'vdsr_c1'),
    ('conv', 64, 1, 3, 1, 1, 0, None, 0, 'vdsr_c1'),
    ('conv', 1, 64, 3, 1, 1, 0, None, 0, 'edsr_c1'),
    ('conv', 64, 256, 3, 1, 1, 0, None, 2, 'edsr_c1'),
    ('conv', 1, 64, 3, 1, 1, 0, 'lrelu', 0, 'lapsrn_c1'),
    ('deconv', 1, 1, 4, 2, 1, 0, None, 0, 'lapsrn_c1'),
    ('conv', 64, 64, 3, 1, 1, 0, 'lrelu', 0, 'lapsrn_c1'),
    ('conv', 1, 64, 9, 1, 4, 0, 'prelu', 0, 'srgan_g_c1'),
    ('conv', 64, 256, 3, 1, 1, 0, 'prelu', 2, 'srgan_g_c1'),
    ('conv', 64, 1, 9, 1, 4, 0, None, 0, 'srgan_g_c1'),
    ('conv', 3, 64, 9, 1, 4, 0, 'prelu', 0, 'srgan_g_c3'),
    ('conv', 1, 64, 5, 1, 0, 0, 'relu', 0, 'espcn_c1_x2'),
    ('conv', 32, 4, 3, 1, 0, 0, None, 2, 'espcn_c1_x2'),
    ('conv', 32, 9, 3, 1, 0, 0, None, 3, 'espcn_c1_x3'),
    ('conv', 32, 16, 3, 1, 0, 0, None, 4, 'espcn_c1_x4'),
    ('conv', 32, 64, 3, 1, 0, 0, None, 8, 'espcn_c1_x8'),
    ('conv', 32, 12, 3, 1, 0, 0, None, 2, 'espcn_c3_x2'),
    ('conv', 32, 27, 3, 1, 0, 0, None, 3, 'espcn_c3_x3'),
    ('conv', 32, 192, 3, 1, 0, 0, None, 8, 'espcn_c3_x8'),
    ('conv', 1, 56, 5, 1, 0, 0, 'prelu', 0, 'fsrcnn_c1_x2'),
    ('conv', 56, 12, 1, 1, 0, 0, 'prelu', 0, 'fsrcnn_c1_x2'),
    ('conv', 12, 56, 1, 1, 0, 0, 'prelu', 0, 'fsrcnn_c1_x2'),
    ('deconv', 56, 1, 9, 2, 3, 1, None, 0, 'fsrcnn_c1_x2'),
    ('deconv', 56, 1, 9, 3, 3, 1, None, 0, 'fsrcnn_c1_x3'),
    ('deconv', 56, 1, 9, 4, 3, 1, None, 0, 'fsrcnn_c1_x4'),
    ('conv', 3, 56, 5, 1, 0, 0, 'prelu', 0, 'fsrcnn_c3_x2'),
    ('deconv', 56, 3, 9, 2, 3, 1, None, 0, 'fsrcnn_c3_x2'),
    ('deconv', 56, 3, 9, 3, 3, 1, None, 0, 'fsrcnn_c3_x3'),
    ('conv', 64, 128, 3, 1, 1, 0, None, 0, 'srgan_d_c1_crop16'),
    ('conv', 128, 128, 3, 2, 1, 0, None, 0, 'srgan_d_c1_crop16'),
    ('conv', 128, 256, 3, 1, 1, 0, None, 0, 'srgan_d_c1_crop16'),
    ('conv', 256, 256, 3, 2, 1, 0, None, 0, 'srgan_d_c1_crop16'),
    ('conv', 256, 512, 3, 1, 1, 0, None, 0, 'srgan_d_c1_crop16'),
    ('linear', 512, 1024, 0, 0, 0, 0, 'lrelu', 0, 'srgan_d_c1_crop16'),
    ('linear', 1024, 1, 0, 0, 0, 0, 'sigmoid', 0, 'srgan_d_c1_crop16'),
    ('linear', 2048, 1024, 0, 0, 0, 0, 'lrelu', 0, 'srgan_d_c1_crop32'),
    ('linear', 4608, 1024, 0, 0, 0, 0, 'lrelu', 0, 'srgan_d_c1_crop48'),
    ('linear', 18432, 1024, 0, 0, 0, 0, 'lrelu', 0, 'srgan_d_c1_crop96'),
]

# (B, In, Out): what the discriminator's layers and tests/test_ops_gpu.py's (5, 96, 20) do not reach
DENSE_EXTRA = [
    (11, 510, 7),       # In % 4 != 0: k_linear_dw's scalar branch; two 8-row batch tiles; Out no multiple of 4 or 8
    (3, 2048, 64),      # linear_wide's boundary, the wide side ...
    (3, 2044, 64),      # ... and the narrow side
    (3, 2048, 1030),    # k_linear_dx_wide's second 1024-row pass
    (3, 8192, 1024),    # crop 64, between the crops of the matrix
    (11, 8192, 1024),
]
DENSE_BATCHES = (3, 11)     # under and over the 8-row (narrow) tile; 11 < 16 leaves the wide tile ragged


def row_id(row):
    kind, cin, cout, k, s, p, op, act, ps = row[:9]
    if kind == "linear":
        return "fc_%d_%d_%s" % (cin, cout, act)
    return "%s%ds%dp%d%s_%d_%d_%s%s" % ("d" if kind == "deconv" else "c", k, s, p, ("o%d" % op) if op else "", cin, cout,
                                        act, ("_ps%d" % ps) if ps else "")


def row_inputs(i):
    """(x, weight in torch's layout, bias, PReLU slope) of conv / deconv row i: two images of 17 x 23 (7 x 9 in front of the
    x8 shuffle), several ragged tiles of every kernel family per image."""
    kind, cin, cout, k, s, p, op, act, ps = LAYER_ROWS[i][:9]
    H, W = (7, 9) if ps == 8 else (17, 23)
    wshape = (cin, cout, k, k) if kind == "deconv" else (cout, cin, k, k)
    w = fill.randn(wshape, 5000 + i, (2.0 / (cin * k * k)) ** 0.5)
    b = fill.randn((cout,), 6000 + i, 0.1)
    x = fill.randn((2, cin, H, W), 7000 + i)
    return x, w, b, torch.tensor([0.25])


def apply_act(z, act, slope=None):
    if act is None:
        return z
    if act == "relu":
        return torch.relu(z)
    if act == "lrelu":
        return F.leaky_relu(z, 0.2)
    if act == "prelu":
        return F.prelu(z, slope.to(z.dtype))
    if act == "tanh":
        return torch.tanh(z)
    if act == "sigmoid":
        return torch.sigmoid(z)
    raise ValueError(act)


def row_linear_part(i, x, w, b):
    """The row's conv / transposed conv without activation and shuffle, in the dtype of its arguments."""
    kind, cin, cout, k, s, p, op, act, ps = LAYER_ROWS[i][:9]
    if kind == "deconv":
        return F.conv_transpose2d(x, w, b, s, p, op)
    return F.conv2d(x, w, b, s, p)


def row_reference(i):
    """fp64 forward of row i with its own epilogue: act(conv), then the pixel shuffle."""
    kind, cin, cout, k, s, p, op, act, ps = LAYER_ROWS[i][:9]
    x, w, b, slope = row_inputs(i)
    y = apply_act(row_linear_part(i, x.double(), w.double(), b.double()), act, slope)
    return F.pixel_shuffle(y, ps) if ps else y
