"""Whole-network and layer parity at every channel count, scale factor and crop size the command line reaches, against
fp64 on the CPU (tables and runners: tests/net_configs_ref.py; conditioning of the inputs: tests/test_net_configs_cpu.py).

Net level: the package net with the oracle's weights, train mode, forward and backward: every output, the input gradient and
every parameter gradient element-wise at the contract's 1e-3, every output max-norm at 1e-4; then the no-grad forward at 1e-4
under the default switches, SRK_BFD_SMALL=0 and SRK_BFW=1, and in the 'bf16x3' precision, where those switches choose among
the library's own kernels (the ones a benchmark-size picture would get), at the contract's 1e-3.  The discriminator is held on its outputs and running statistics; its gradients are held at layer level (see
test_discriminator_forward_and_running_statistics).

Layer level: the conv / transposed-conv / linear layers these configurations add to what tests/test_ops_gpu.py runs
(net_configs_ref.LAYER_ROWS), forward with the layer's own epilogue and backward without activation, on ragged tiles.

Every test prints what it measured as `PARITY ...` lines (pytest -s): profiles/net_configs_parity.txt is one such run."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import net_configs_ref as N
from conftest import TOL_CONTRACT, TOL_TIGHT, assert_close_elementwise, rel_err
from oracle import fill

pytestmark = pytest.mark.gpu

# environment switches of the no-grad forward: test_ops_gpu.VARIANTS' auto_lds_weights and auto_wave_specialized.  On a
# small problem run_gather (csrc/api.hip) asks k_conv_bfd's small-problem blocks before k_conv_bfw, so SRK_BFW=1 alone leaves
# these shapes where they were; with SRK_BF3_DIRECT=0 (test_conv_wave_specialized_channel_slices' pair) the library's own
# choice does reach the wave-specialised kernels.
SWITCHES = {"default": {}, "lds_weights": {"SRK_BFD_SMALL": "0"}, "wave_specialized": {"SRK_BFW": "1"}}
SWITCHES_AUTO = dict(SWITCHES, wave_specialized_forced={"SRK_BFW": "1", "SRK_BF3_DIRECT": "0"})
CONV_ROWS = [i for i, r in enumerate(N.LAYER_ROWS) if r[0] != "linear"]
LINEAR_ROWS = [i for i, r in enumerate(N.LAYER_ROWS) if r[0] == "linear"]


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    _pkg().ops.set_precision("mixed")


def _ids(rows):
    return [N.row_id(N.LAYER_ROWS[i]) for i in rows]


# ---- net level ------------------------------------------------------------------------------------------------------------
class _KernelLog(object):
    """Reads srk_last_kernel_name() behind every conv / transposed-conv module's launch (the blocks call `run`, so that is
    what is wrapped) and keeps one line per distinct (layer shape, kernel).  The library records no name for linear layers:
    their family follows from the shape alone (linear_wide, csrc/bn_linear.hip)."""

    def __init__(self, pkg, net):
        self.lib, self.lines, self.taps = pkg._lib.load(), {}, []
        L = pkg.layers
        for m in net.modules():
            if isinstance(m, (L.Conv2d, L.ConvTranspose2d)):
                kind = "deconv" if isinstance(m, L.ConvTranspose2d) else "conv"
                what = "%s %d->%d %dx%d s%d p%d" % (kind, m.in_channels, m.out_channels, m.kernel_size[0], m.kernel_size[1],
                                                    m.stride[0], m.padding[0])
                m.run = self._wrap(m.run, what)
                self.taps.append(m)
            elif isinstance(m, L.Linear):
                wide = m.in_features % 4 == 0 and m.in_features >= 2048 and m.out_features >= 64
                self.lines[("linear %d->%d" % (m.in_features, m.out_features),
                            "k_linear_fwd_wide (by shape)" if wide else "k_linear_fwd (by shape)")] = None

    def _wrap(self, run, what):
        def tapped(*args, **kwargs):
            y = run(*args, **kwargs)
            self.lines[(what, self.lib.srk_last_kernel_name().decode())] = None
            return y
        return tapped

    def flush(self, head):
        for what, kern in self.lines:
            print("PARITY %s: layer %s -> %s" % (head, what, kern))
        self.lines = {k: None for k in self.lines if k[0].startswith("linear")}

    def close(self):
        for m in self.taps:
            del m.run


def _assert_rows(rows):
    for what, bar, used in rows:
        assert (used <= 1.0) if bar.startswith("elementwise") else (used < 1.0), (what, bar, used)


def _report(name, stage, rows):
    what, bar, used = N.worst(rows)
    print("PARITY %s %s: %d checks, worst %.4f of its bar (%s, %s)" % (name, stage, len(rows), used, what, bar))
    for kind in sorted({r[1] for r in rows}):
        w = N.worst([r for r in rows if r[1] == kind])
        print("PARITY %s %s:   %-24s worst %.4f of the bar (%s)" % (name, stage, kind, w[2], w[0]))


def _product_net(gpu, cfg):
    pkg = _pkg()
    net = getattr(pkg, cfg.product)(*cfg.args)
    net.load_state_dict(N.make_oracle(cfg).state_dict())
    return net.to(gpu).train()


def _no_grad_forwards(monkeypatch, name, net, x, ref, log):
    """The no-grad forward against the oracle's eval-mode outputs: in the default precision ('mixed': the fp32-faithful
    class) under the three switch sets at TOL_FWD; then in the 'bf16x3' precision, where the switches choose among the
    library's own kernels (what a benchmark-size picture gets), at the contract's 1e-3 -- the bar of the fastest mode, whose
    ~5e-6 per layer adds up over 20 layers."""
    if ref.buffers:
        net.eval()      # the BatchNorm nets: after the training forward has moved the running statistics
    ops = _pkg().ops
    for precision, switches, tol in (("mixed", SWITCHES, N.TOL_FWD), ("bf16x3", SWITCHES_AUTO, TOL_CONTRACT)):
        ops.set_precision(precision)
        for tag, env in switches.items():
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            with torch.no_grad():
                outs = N._as_list(net(x))
            for k in env:
                monkeypatch.delenv(k)
            head = "%s no-grad %s %s" % (name, precision, tag)
            log.flush(head)
            assert len(outs) == len(ref.eval_outs)
            errs = [rel_err(a, b.float()) for a, b in zip(outs, ref.eval_outs)]
            print("PARITY %s: max-norm %s (bar %.0e)" % (head, ", ".join("%.3e" % e for e in errs), tol))
            assert max(errs) < tol, (head, errs)
    ops.set_precision("mixed")


@pytest.mark.parametrize("name", N.NET_CONFIGS)
def test_config_matches_fp64_oracle(gpu, monkeypatch, name):
    """Train-mode forward and backward, compared exactly as test_nets_gpu.test_net_elementwise_outputs_and_body_gradients
    does (net_configs_ref.compare), against the oracle in fp64; then the three no-grad forwards."""
    pkg = _pkg()
    cfg = N.CONFIGS[name]
    ref = N.run_oracle(name)
    net = _product_net(gpu, cfg)
    log = _KernelLog(pkg, net)
    try:
        x = fill.rand(cfg.ishape, N.SEED_X).to(gpu).requires_grad_(True)
        outs = N._as_list(net(x))
        log.flush(name + " train")
        assert len(outs) == len(ref.outs)
        torch.autograd.backward(outs, [g.to(gpu) for g in N.out_grads(ref.outs)])
        grads = {}
        for k, p in net.named_parameters():
            assert p.grad is not None, k
            grads[k] = p.grad.detach().cpu()
        assert set(grads) == set(ref.grads)
        got = N.Ref([y.detach().cpu() for y in outs], x.grad.detach().cpu(), {k: grads[k] for k in ref.grads},
                    {k: b.detach().cpu() for k, b in net.named_buffers()}, [])
        rows = N.compare(name, got, ref)
        _report(name, "train", rows)
        _assert_rows(rows)
        _no_grad_forwards(monkeypatch, name, net, x.detach(), ref, log)
    finally:
        log.close()


@pytest.mark.parametrize("name", N.DISC_CONFIGS)
def test_discriminator_forward_and_running_statistics(gpu, monkeypatch, name):
    """SRGAN's discriminator at every crop size (its dense layer is 512 (crop / 16)^2 -> 1024) and channel count: the
    train-mode output, the BatchNorm running statistics after that forward and the eval-mode output, at the bars above.

    Its gradients are NOT compared at net level.  With (5, 1, 48, 48) on the CPU the fp64 oracle has a BatchNorm output of
    2.85e-7 in conv_blocks.5; the fp32 oracle rounds it across zero, the LeakyReLU behind it flips, and the gradient of
    conv_blocks.5.conv.weight differs by 0.29 of its maximum between fp32 and fp64 -- plain torch against itself.  Batch 2 at
    crop 96, batch 8 at crop 16 and batch 5 at crop 96 fail the same way.  The last maps are 1 x 1 to 6 x 6, so one unit
    carries a large share of the gradient, and no seed can be screened for a safe margin: with about 3e5 BatchNorm outputs per
    sample some unit always lies within rounding of zero.  So every kernel of its backward is held at layer level instead
    (test_layer_backward, test_layer_masked_data_gradient, test_dense_layer: the mask is data there, kernel and reference
    cannot disagree on a sign), and the 3-channel crop-32 gradients stay where they were (test_nets_gpu.py's srgan_d)."""
    pkg = _pkg()
    cfg = N.CONFIGS[name]
    ref = N.run_oracle(name, False)
    net = _product_net(gpu, cfg)
    log = _KernelLog(pkg, net)
    try:
        x = fill.rand(cfg.ishape, N.SEED_X).to(gpu)
        outs = N._as_list(net(x.clone().requires_grad_(True)))      # the training forward (saves for backward)
        log.flush(name + " train")
        got = N.Ref([y.detach().cpu() for y in outs], None, {}, {k: b.detach().cpu() for k, b in net.named_buffers()}, [])
        rows = N.compare(name, got, ref)
        assert len(rows) == 2 + 4 * 7          # one output, running mean and variance of seven BatchNorms, each on two bars
        _report(name, "train", rows)
        _assert_rows(rows)
        _no_grad_forwards(monkeypatch, name, net, x, ref, log)
    finally:
        log.close()


# ---- layer level: convs and transposed convs --------------------------------------------------------------------------------
def _act_code(pkg, act):
    L = pkg._lib
    return {None: L.ACT_NONE, "relu": L.ACT_RELU, "prelu": L.ACT_PRELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH,
            "sigmoid": L.ACT_SIGMOID}[act]


def _row_cfg(pkg, row, act, ps, algo):
    kind, cin, cout, k, s, p, op = row[:7]
    return pkg.ops.ConvCfg(s, p, kind == "deconv", op, _act_code(pkg, act), 0.2 if act == "lrelu" else 0.0, ps, algo)


_REFS = {}


def _row_reference(i):
    if i not in _REFS:
        _REFS[i] = N.row_reference(i).float()
    return _REFS[i]


@pytest.mark.parametrize("algo", ["auto", "bf16x6"])
@pytest.mark.parametrize("switch", list(SWITCHES_AUTO))
@pytest.mark.parametrize("i", CONV_ROWS, ids=_ids(CONV_ROWS))
def test_layer_forward(gpu, monkeypatch, i, switch, algo):
    """ops.conv2d_infer with the layer's own epilogue (bias, activation, fused pixel shuffle) against torch fp64, under the
    default switches, SRK_BFD_SMALL=0, SRK_BFW=1 and SRK_BFW=1 with SRK_BF3_DIRECT=0.  `auto` is the library's own choice
    (the 'bf16x3' precision hands SRK_ALGO_AUTO through; 'mixed' would turn it into bf16x6): 1e-4 max-norm, 1e-3 element-wise;
    `bf16x6` is the fp32-faithful class: TOL_TIGHT and 1e-4 (the bars of test_conv_rows_on_n_kernel).  A fused shuffle
    must not change values: when the same kernel ran the layer without the shuffle, the two outputs agree bit for bit."""
    pkg = _pkg()
    ops, lib = pkg.ops, pkg._lib.load()
    for k, v in SWITCHES_AUTO[switch].items():
        monkeypatch.setenv(k, v)
    row = N.LAYER_ROWS[i]
    act, ps = row[7], row[8]
    if algo == "auto":
        ops.set_precision("bf16x3")
        code = 0
    else:
        code = pkg._lib.ALGO_MFMA_BF16X6
    x, w, b, slope = (t.to(gpu) for t in N.row_inputs(i))
    pw = slope if act == "prelu" else None
    ref = _row_reference(i)
    with torch.no_grad():
        y = ops.conv2d_infer(x, w, b, None, _row_cfg(pkg, row, act, ps, code), pw)
        name = lib.srk_last_kernel_name().decode()
        y2 = ops.conv2d_infer(x, w, b, None, _row_cfg(pkg, row, act, ps, code), pw)
    assert tuple(y.shape) == tuple(ref.shape)
    tol, rtol = (1e-4, 1e-3) if algo == "auto" else (TOL_TIGHT, 1e-4)
    err = rel_err(y, ref)
    print("PARITY layer %s forward %s %s: %s max-norm %.3e (bar %.0e), element-wise %.4f of the %.0e bar"
          % (N.row_id(row), algo, switch, name, err, tol, N.bar_elementwise(y, ref, rtol), rtol))
    assert torch.equal(y, y2)                   # fixed summation order: run-to-run identical
    assert err < tol
    assert_close_elementwise(y, ref, rtol, what=N.row_id(row))
    if ps:
        with torch.no_grad():
            plain = ops.conv2d_infer(x, w, b, None, _row_cfg(pkg, row, act, 0, code), pw)
        plain_name = lib.srk_last_kernel_name().decode()
        same = plain_name == name
        print("PARITY layer %s forward %s %s: without the shuffle %s -> %s" % (
            N.row_id(row), algo, switch, plain_name, "compared bit for bit" if same else "another kernel, not compared"))
        assert rel_err(F.pixel_shuffle(plain, ps), ref) < tol
        if same:
            assert torch.equal(y, F.pixel_shuffle(plain, ps))


FEW_OUT = [i for i in CONV_ROWS if N.LAYER_ROWS[i][0] == "conv" and N.LAYER_ROWS[i][2] <= 3 and N.LAYER_ROWS[i][1] in (32, 64)
           and N.LAYER_ROWS[i][4] == 1 and not N.LAYER_ROWS[i][8]]


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("i", FEW_OUT, ids=_ids(FEW_OUT))
def test_single_output_channel_kernel_family(gpu, monkeypatch, i, mode):
    """The Cout = 1 reconstruction convs under SRK_ROWN=2, where run_gather's choice follows from the shape alone: more taps
    than one 32-column group on k_conv_rown, the others on k_conv_tapn (as test_conv_few_output_channels asserts for 2 and 3
    output channels)."""
    pkg = _pkg()
    ops, lib = pkg.ops, pkg._lib.load()
    monkeypatch.setenv("SRK_ROWN", "2")
    row = N.LAYER_ROWS[i]
    kind, cin, cout, k = row[:4]
    x, w, b, slope = (t.to(gpu) for t in N.row_inputs(i))
    code = {"bf16x3": 4, "bf16x6": pkg._lib.ALGO_MFMA_BF16X6}[mode]
    with torch.no_grad():
        y = ops.conv2d_infer(x, w, b, None, _row_cfg(pkg, row, row[7], 0, code))
    name = lib.srk_last_kernel_name().decode()
    assert name.startswith("k_conv_rown<" if k * k * cout > 32 else "k_conv_tapn<"), name
    ref = _row_reference(i)
    tol, rtol = (1e-4, 1e-3) if mode == "bf16x3" else (TOL_TIGHT, 1e-4)
    print("PARITY layer %s forward %s rown: %s max-norm %.3e (bar %.0e)" % (N.row_id(row), mode, name, rel_err(y, ref), tol))
    assert rel_err(y, ref) < tol
    assert_close_elementwise(y, ref, rtol, what=N.row_id(row))


def _grad_bars(tag, pairs):
    for what, a, b in pairs:
        err = rel_err(a, b.float())
        print("PARITY layer %s backward: %s max-norm %.3e (bar 1e-04), element-wise %.4f of the 1e-03 bar"
              % (tag, what, err, N.bar_elementwise(a, b, 1e-3)))
    for what, a, b in pairs:
        assert rel_err(a, b.float()) < 1e-4, (tag, what)
        assert_close_elementwise(a, b.float(), 1e-3, what="%s %s" % (tag, what))


@pytest.mark.parametrize("i", CONV_ROWS, ids=_ids(CONV_ROWS))
def test_layer_backward(gpu, i):
    """dx, dw and db of ops.conv2d(...).backward against fp64 autograd, without activation (no sign decision separates
    kernel and reference), the fused pixel shuffle included: 1e-4 max-norm (test_conv_few_output_channels_backward,
    test_deconv_large_halo_small_problem) and 1e-3 element-wise."""
    pkg = _pkg()
    ops, lib = pkg.ops, pkg._lib.load()
    row = N.LAYER_ROWS[i]
    ps = row[8]
    x, w, b, slope = N.row_inputs(i)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = N.row_linear_part(i, xr, wr, br)
    if ps:
        ref = F.pixel_shuffle(ref, ps)
    g = fill.randn(tuple(ref.shape), 8000 + i)
    ref.backward(g.double())
    xg, wg, bg = (t.to(gpu).requires_grad_(True) for t in (x, w, b))
    y = ops.conv2d(xg, wg, bg, None, _row_cfg(pkg, row, None, ps, 0))
    name = lib.srk_last_kernel_name().decode()
    assert tuple(y.shape) == tuple(ref.shape)
    y.backward(g.to(gpu))
    print("PARITY layer %s backward: forward kernel %s" % (N.row_id(row), name))
    _grad_bars(N.row_id(row), [("y", y, ref.detach()), ("dx", xg.grad, xr.grad), ("dw", wg.grad, wr.grad),
                               ("db", bg.grad, br.grad)])


MASKED = [i for i in CONV_ROWS if N.LAYER_ROWS[i][0] == "conv" and N.LAYER_ROWS[i][7] in ("relu", "lrelu")
          and not N.LAYER_ROWS[i][8]]


@pytest.mark.parametrize("i", MASKED, ids=_ids(MASKED))
def test_layer_masked_data_gradient(gpu, i):
    """The data gradient of a layer with ReLU / LeakyReLU behind it takes that activation's mask on dy.  The mask is DATA
    here, as in test_conv_image_gradient_with_mask: an output tensor with |y| >= 0.1 and seeded signs, handed to the kernel
    and to the reference alike, so the two cannot disagree on a sign."""
    pkg = _pkg()
    ops, L = pkg.ops, pkg._lib
    lib = L.load()
    row = N.LAYER_ROWS[i]
    slope = 0.2 if row[7] == "lrelu" else 0.0
    x, w, b, _ = N.row_inputs(i)
    xr = x.double().requires_grad_(True)
    lin = N.row_linear_part(i, xr, w.double(), None)
    g = fill.randn(tuple(lin.shape), 8000 + i)
    sgn = fill.randn(tuple(lin.shape), 9000 + i)
    ymask = torch.where(sgn >= 0, 0.1 + sgn.abs(), -0.1 - sgn.abs())
    lin.backward(g.double() * torch.where(ymask > 0, 1.0, slope).double())
    cfg = _row_cfg(pkg, row, None, 0, 0)
    d = ops._make_desc(x.shape, w, cfg, "bwd")
    dy = g.to(gpu).contiguous(memory_format=torch.channels_last)
    yg = ymask.to(gpu).contiguous(memory_format=torch.channels_last)
    wpb = ops.pack_weight_bwd(w.to(gpu), False, 0)
    dx = torch.full(tuple(x.shape), float("nan"), device=gpu).contiguous(memory_format=torch.channels_last)
    mask = L.BwdMask(L.ptr(yg), slope)
    rc = lib.srk_conv2d_backward_data(ctypes.byref(d), L.ptr(dy), L.ptr(wpb), L.ptr(dx), ctypes.byref(mask), None,
                                      L.stream_ptr())
    assert rc == 0, lib.srk_last_error_string()
    print("PARITY layer %s masked dx: kernel %s" % (N.row_id(row), lib.srk_last_kernel_name().decode()))
    _grad_bars(N.row_id(row) + " masked", [("dx", dx, xr.grad)])


# ---- layer level: dense layers ----------------------------------------------------------------------------------------------
DENSE = [(b, N.LAYER_ROWS[i][1], N.LAYER_ROWS[i][2]) for i in LINEAR_ROWS for b in N.DENSE_BATCHES] + list(N.DENSE_EXTRA)
DENSE_ACTS = (None, "relu", "lrelu", "tanh", "sigmoid")     # srk_linear_forward refuses PReLU (applied unfused)
DENSE_BAR = 2e-6                                            # test_linear_wide_layers' bar


@pytest.mark.parametrize("shape", DENSE, ids=["b%d_%d_%d" % s for s in DENSE])
def test_dense_layer(gpu, shape):
    """srk_linear_forward / srk_linear_backward against float64 matmuls, element-wise at 2e-6: the forward with every
    activation the entry point accepts, dx alone (dw = NULL: the frozen-parameter call), dw / db with beta = 0 and
    accumulated into seeded buffers.  The gradient calls carry no activation."""
    pkg = _pkg()
    ops, L = pkg.ops, pkg._lib
    lib = L.load()
    B, In, Out = shape
    x = fill.randn((B, In), 71)
    w = fill.randn((Out, In), 72) * 0.02
    b = fill.randn((Out,), 73)
    g = fill.randn((B, Out), 74)
    z = x.double() @ w.double().t() + b.double()
    xg, wg, bg, gg = (t.to(gpu) for t in (x, w, b, g))
    wide = In % 4 == 0 and In >= 2048 and Out >= 64
    tag = "dense b%d %d->%d (%s kernels by shape)" % (B, In, Out, "wide" if wide else "narrow")
    checks = []
    for act in DENSE_ACTS:
        y = ops.linear(xg, wg, bg, _act_code(pkg, act), 0.2 if act == "lrelu" else 0.0)
        checks.append(("forward " + str(act), y, N.apply_act(z, act)))
    dx_ref, dw_ref, db_ref = g.double() @ w.double(), g.double().t() @ x.double(), g.double().sum(0)

    def backward(dx, dw, db, beta):
        rc = lib.srk_linear_backward(L.ptr(xg), L.ptr(wg), L.ptr(gg), L.ptr(dx), L.ptr(dw), L.ptr(db), B, In, Out, beta,
                                     L.stream_ptr())
        assert rc == 0, lib.srk_last_error_string()

    nan = lambda *s: torch.full(s, float("nan"), device=gpu)
    dx = nan(B, In)
    backward(dx, None, None, 0.0)
    checks.append(("dx alone", dx, dx_ref))
    dx2, dw, db = nan(B, In), nan(Out, In), nan(Out)
    backward(dx2, dw, db, 0.0)
    checks += [("dx", dx2, dx_ref), ("dw", dw, dw_ref), ("db", db, db_ref)]
    sw, sb = fill.randn((Out, In), 75), fill.randn((Out,), 76)
    dwa, dba = sw.to(gpu), sb.to(gpu)
    backward(None, dwa, dba, 1.0)
    checks += [("dw accumulated", dwa, sw.double() + dw_ref), ("db accumulated", dba, sb.double() + db_ref)]
    print("PARITY %s: share of the 2e-06 element-wise bar: %s"
          % (tag, ", ".join("%s %.3f" % (what, N.bar_elementwise(a, r, DENSE_BAR)) for what, a, r in checks)))
    for what, a, r in checks:
        assert_close_elementwise(a, r, DENSE_BAR, what="%s %s" % (tag, what))
    assert torch.equal(dx2, dx)
