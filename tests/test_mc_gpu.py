"""The motion-compensation kernels (csrc/mc.hip) on the device against the fp64 restatement of tests/mc_ref.py: the whole
case table with the flow in both memory formats, under the unit seed, a declared seed and a foreign upstream gradient;
exact properties (zero flow, constant flow); repeatability, eagerly and from a replayed graph.

Bars: the project's contract, outputs and losses 1e-4 max|ref|, gradients 1e-3 max|ref|, + 1e-9 where the reference can
be 0 (mc_ref.bar_out / bar_grad).  No element is left out: the table's coordinates are exact in fp32, so fp32 and fp64
pick the same cell everywhere, on the integers included."""
import numpy as np
import pytest
import torch

import mc_ref as R

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def ops(gpu):
    import pytorch_super_resolution_model_collection_amd as p
    return p.ops


def dev(a, gpu, last=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t.contiguous(memory_format=CL) if last else t


def host(t):
    return t.detach().cpu().double().numpy()


def close(got, want, bar, what):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    err = float(np.abs(got - want).max())
    print("%-28s err %.3e bar %.3e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("last", [False, True], ids=["flow_nchw", "flow_nhwc"])
@pytest.mark.parametrize("shape,family", R.cases(), ids=str)
def test_motion_fuse_against_the_restatement(ops, gpu, shape, family, last):
    n, c, h, w = shape
    frames, flow = R.case(shape, family)
    g = np.random.RandomState(11).randn(n, 3 * c, h, w).astype(np.float32)
    fr = dev(frames, gpu)

    def run(declared=None):
        fl = dev(flow, gpu, last).requires_grad_(True)
        if declared is None:
            return (fl,) + ops.motion_fuse(fr, fl)
        with ops.loss_seed(*declared):
            return (fl,) + ops.motion_fuse(fr, fl)

    want_fused, want_mc, want_d = R.motion_fuse(frames, flow)
    # the unit seed
    fl, fused, mc = run()
    assert fused.shape == (n, 3 * c, h, w) and fused.is_contiguous(memory_format=CL) and mc.shape == ()
    close(fused, want_fused, R.bar_out(want_fused), "fused")
    close(mc, want_mc, R.bar_out(want_mc), "mc")
    ops.backward(mc)
    close(fl.grad, want_d, R.bar_grad(want_d), "dflow unit seed")
    # a declared seed
    seed = torch.full((), 0.25, device=gpu)
    fl, fused, mc = run((0.25, seed))
    ops.backward(mc, seed)
    want = R.motion_fuse(frames, flow, None, 0.25)[2]
    close(fl.grad, want, R.bar_grad(want), "dflow declared seed")
    # a foreign upstream gradient on both outputs, with and without a declared seed
    want = R.motion_fuse(frames, flow, g, 0.6)[2]
    for declared in (None, (0.25, seed)):
        fl, fused, mc = run(declared)
        torch.autograd.backward([fused, mc], [dev(g, gpu, True), torch.full((), 0.6, device=gpu)])
        close(fl.grad, want, R.bar_grad(want), "dflow foreign")
    # ... and an NCHW gradient of the fused tensor alone
    fl, fused, mc = run()
    fused.backward(dev(g, gpu))
    want = R.motion_fuse(frames, flow, g, 0.0)[2]
    close(fl.grad, want, R.bar_grad(want), "dflow fused only")


@pytest.mark.parametrize("shape,family", R.cases(), ids=str)
def test_flow_warp_against_the_restatement(ops, gpu, shape, family):
    n, c, h, w = shape
    frames, flow = R.case(shape, family)
    img, fl_np = frames[:, 2], flow[n:]
    g = np.random.RandomState(12).randn(n, c, h, w).astype(np.float32)
    want, want_d = R.warp(img, fl_np, g)
    for img_last in (False, True):
        for flow_last in (False, True):
            fl = dev(fl_np, gpu, flow_last).requires_grad_(True)
            out = ops.flow_warp(dev(img, gpu, img_last), fl)
            assert out.is_contiguous(memory_format=CL)
            close(out, want, R.bar_out(want), "warp")
            out.backward(dev(g, gpu, flow_last))
            close(fl.grad, want_d, R.bar_grad(want_d), "warp dflow")


@pytest.mark.parametrize("mhw", [(1, 1, 1), (2, 1, 5), (2, 7, 9), (16, 48, 48)], ids=str)
def test_flow_huber_against_the_restatement(ops, gpu, mhw):
    m, h, w = mhw
    flow = np.random.RandomState(3).randn(m, 2, h, w).astype(np.float32)
    want_l, want_g = R.flow_huber(flow, 0.01)
    seed = torch.full((), 0.5, device=gpu)
    for last in (False, True):
        fl = dev(flow, gpu, last).requires_grad_(True)
        loss = ops.flow_huber_loss(fl)
        close(loss, want_l, R.bar_out(want_l), "huber")
        ops.backward(loss)
        close(fl.grad, want_g, R.bar_grad(want_g), "huber grad unit")
        fl = dev(flow, gpu, last).requires_grad_(True)
        with ops.loss_seed(0.5, seed):
            loss = ops.flow_huber_loss(fl, eps=0.01)
        ops.backward(loss, seed)
        close(fl.grad, 0.5 * want_g, R.bar_grad(0.5 * want_g), "huber grad declared")
        fl = dev(flow, gpu, last).requires_grad_(True)
        (ops.flow_huber_loss(fl) * 3.0).backward()
        close(fl.grad, 3.0 * want_g, R.bar_grad(3.0 * want_g), "huber grad foreign")
    # the table's flows too (exact quarter steps give exactly repeated differences)
    _, flow = R.case((2, 3, 7, 9), "quarter")
    want_l, want_g = R.flow_huber(flow, 0.01)
    fl = dev(flow, gpu).requires_grad_(True)
    loss = ops.flow_huber_loss(fl)
    ops.backward(loss)
    close(loss, want_l, R.bar_out(want_l), "huber table")
    close(fl.grad, want_g, R.bar_grad(want_g), "huber table grad")


def test_zero_flow_copies_the_frames(ops, gpu):
    frames, _ = R.case((3, 3, 32, 32), "odd128")
    fr = dev(frames, gpu)
    fused, mc = ops.motion_fuse(fr, torch.zeros(6, 2, 32, 32, device=gpu))
    assert torch.equal(fused, fr.reshape(3, 9, 32, 32))
    want = ((frames[:, [0, 2]].astype(np.float64) - frames[:, 1:2]) ** 2).mean()
    close(mc, want, R.bar_out(want), "mc at zero flow")
    assert torch.equal(ops.flow_warp(fr[:, 0], torch.zeros(3, 2, 32, 32, device=gpu)), fr[:, 0])


def test_constant_flow_is_smooth(ops, gpu):
    fl = torch.full((2, 2, 7, 9), 1.25, device=gpu, requires_grad=True)
    loss = ops.flow_huber_loss(fl, eps=0.01)
    ops.backward(loss)
    close(loss, np.sqrt(0.01), 1e-4 * 0.1, "huber of a constant flow")
    assert torch.count_nonzero(fl.grad).item() == 0


def _everything(ops, fr, flow, g):
    fl = flow.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    fused, mc = ops.motion_fuse(fr, fl)
    hub = ops.flow_huber_loss(fl)
    torch.autograd.backward([fused, mc, hub], [g, ops.unit_seed(fr.device), ops.unit_seed(fr.device)])
    return fused.detach(), mc.detach(), hub.detach(), fl.grad


def test_two_calls_and_a_replayed_graph_give_the_same_bits(ops, gpu):
    frames, flow = R.case((3, 3, 32, 32), "odd128")
    fr, fl = dev(frames, gpu), dev(flow, gpu, True)
    g = dev(np.random.RandomState(1).randn(3, 9, 32, 32).astype(np.float32), gpu, True)
    first = _everything(ops, fr, fl, g)
    second = _everything(ops, fr, fl, g)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # the forward and the backward launches in one graph, replayed twice
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused, mc = ops.motion_fuse(fr, fl)       # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    flg = fl.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        fused, mc = ops.motion_fuse(fr, flg)
        hub = ops.flow_huber_loss(flg)
        grads = torch.autograd.grad([fused, mc, hub], [flg], [g, ops.unit_seed(gpu), ops.unit_seed(gpu)])
    for _ in range(2):
        fused.zero_(), mc.zero_(), grads[0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (fused, mc, hub, grads[0])):
            assert torch.equal(a, b)


def test_refusals(ops, gpu):
    fr = torch.zeros(1, 3, 1, 4, 4, device=gpu)
    fl = torch.zeros(2, 2, 4, 4, device=gpu)
    with pytest.raises(ValueError, match="`frames` requires a gradient"):
        ops.motion_fuse(fr.clone().requires_grad_(True), fl)
    with pytest.raises(ValueError, match="`img` requires a gradient"):
        ops.flow_warp(fr[:, 0].clone().requires_grad_(True), fl[:1])
    with pytest.raises(ValueError, match=r"flow must be fp32 \[2,2,4,4\]"):
        ops.motion_fuse(fr, fl[:1])
    with pytest.raises(ValueError, match=r"frames must be a non-empty fp32 \[N,3,C,H,W\]"):
        ops.motion_fuse(fr[:, :2], fl)
    with pytest.raises(ValueError, match="eps 0.0 is not positive"):
        ops.flow_huber_loss(fl, eps=0.0)
