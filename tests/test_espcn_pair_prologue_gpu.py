"""k_espcn_pair's prologue and dead rows (csrc/conv_pair.hip): max|x| measured inside the launch, the first layer's
operands prepared once per filter, and the skipped work of a column's short last tile.  All of it must leave every output
bit where the separate srk_absmax pass, the in-kernel weight preparation and the full tile put it."""
import copy

import pytest
import torch

from pytorch_super_resolution_model_collection_amd import _lib, models, ops

pytestmark = pytest.mark.gpu


def _net(seed=0):
    """The weights test_espcn_pair_walk_gpu uses: ESPCN's own initialisation and non-zero biases (the bound of the
    intermediate sees them)."""
    torch.manual_seed(seed)
    net = models.ESPCNNet(3, 64, 4).cuda()
    net.weight_init()
    with torch.no_grad():
        for b in (net.layers[0].conv.bias, net.layers[1].conv.bias):
            b.uniform_(-0.05, 0.05)
    return net.eval()


def _ref64(net, x):
    c1, c2 = net.layers[0].conv, net.layers[1].conv
    y = torch.relu(torch.nn.functional.conv2d(x.double(), c1.weight.double(), c1.bias.double()))
    return torch.relu(torch.nn.functional.conv2d(y, c2.weight.double(), c2.bias.double()))


def _err(y, ref):
    d = (y.double() - ref).abs()
    scale = ref.abs().max().item()
    return d.max().item() / scale, d.pow(2).mean().sqrt().item() / scale


def _no_timeouts():
    torch.cuda.synchronize()
    assert _lib.load().srk_ring_timeouts(1) == 0


def _pair(net, x, scan=False):
    y = ops.espcn_pair(x, net.layers[0], net.layers[1], force=True, scan=scan)
    assert y is not None
    assert _lib.load().srk_last_kernel_name().decode() == "k_espcn_pair"
    return y


def _grid(shape):
    n, h, w = shape
    tiles = n * ((h - 6 + 7) // 8) * ((w - 6 + 15) // 16)
    return min(tiles, torch.cuda.get_device_properties(0).multi_processor_count)


def _input(case):
    """(1, 14, 22): one tile, one block.  (2, 86, 486): 600 tiles on as many blocks as the device has CUs, runs of 2 - 3
    tiles that start inside columns.  (3, 47, 61) "neg": scaled by 3.7 and one element set to -9.0 -- the maximum is a
    negative value that one block's slice holds.  (1, 7, 7): 147 elements, 36 float4s and a tail of three."""
    shape, neg = case
    n, h, w = shape
    torch.manual_seed(6)
    x = torch.rand(n, 3, h, w, device="cuda")
    if neg:
        x *= 3.7
        x.view(-1)[x.numel() // 3 + 5] = -9.0
    return x


CASES = [((1, 14, 22), False), ((2, 86, 486), False), ((3, 47, 61), True), ((1, 7, 7), False)]


@pytest.mark.parametrize("scan", [False, True], ids=["rendezvous", "scan"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + ("neg" if c[1] else ""))
def test_in_launch_max_equals_the_pass(case, scan):
    net = _net()
    x = _input(case)
    xc = x.clone()
    lib = _lib.load()
    assert lib.srk_ring_timeouts(1) >= 0 and lib.srk_espcn_pair_scans(1) >= 0
    with torch.no_grad():
        assert getattr(x, "_srk_amax", None) is None
        a = _pair(net, x, scan=scan)
        slots_pass = ops.amax_of(xc)      # the separate pass
        b = _pair(net, xc)
    assert torch.equal(a, b)
    slots = ops.amax_of(x, compute=False)   # what the launch left: x's tag
    assert slots is not None and slots.data_ptr() != slots_pass.data_ptr()
    assert slots.max().item() == x.abs().max().item() == slots_pass.max().item()
    assert slots[1].item() == 0.0 and slots[2].item() == 0.0   # the rendezvous' counter words, back at zero
    if case[1]:
        assert slots.max().item() == 9.0
    with torch.no_grad():   # a second call with the same tensor object reuses the tag
        c = _pair(net, x)
    assert ops.amax_of(x, compute=False).data_ptr() == slots.data_ptr() and torch.equal(a, c)
    torch.cuda.synchronize()
    scans = lib.srk_espcn_pair_scans(1)
    print("case %s scan %s: blocks on the scan path %d of %d" % (case, scan, scans, _grid(case[0])))
    # One block per CU and at most as many blocks as CUs: every block is resident, so the rendezvous completes and no
    # block may have run into its cap (the output would be the same bits, some 25 ms late).
    assert scans == (_grid(case[0]) if scan else 0)
    _no_timeouts()


def test_captured_launch_replays_with_a_running_maximum():
    """The slots come from a chunk zeroed BEFORE the capture, so nothing zeroes the counter words between replays but the
    kernel itself, and the slots keep the running maximum of the fills."""
    net = _net()
    shape = (2, 3, 86, 486)
    torch.manual_seed(7)
    fills = [torch.rand(shape, device="cuda") * s for s in (0.9, 2.5, 7.0)]
    static = torch.zeros(shape, device="cuda")
    lib = _lib.load()
    assert lib.srk_espcn_pair_scans(1) >= 0
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.no_grad():
        _pair(net, torch.rand(shape, device="cuda"))   # filters prepared, a zeroed chunk of slots at hand
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                y = _pair(net, static)
        running = 0.0
        for f in fills:
            static.copy_(f)
            g.replay()
            torch.cuda.synchronize()
            assert f.abs().max().item() > running   # a LARGER maximum each time
            running = max(running, f.abs().max().item())
            ref = _pair(net, ops.declare_absmax(f.clone(), running))
            assert torch.equal(y, ref)
    torch.cuda.synchronize()
    assert lib.srk_espcn_pair_scans(1) == 0   # every replay's rendezvous completed: the counters were back at zero
    _no_timeouts()


def test_prepared_first_layer_follows_the_weights():
    torch.manual_seed(8)
    x = torch.rand(2, 3, 47, 61, device="cuda")
    neta, netb = _net(0), _net(1)
    with torch.no_grad():
        a0, b0 = _pair(neta, x), _pair(netb, x)
        assert not torch.equal(a0, b0)
        # two nets used alternately keep their own prepared filters
        assert torch.equal(_pair(neta, x), a0) and torch.equal(_pair(netb, x), b0) and torch.equal(_pair(neta, x), a0)
        # an in-place change is seen by the next call
        neta.layers[0].conv.weight.mul_(1.5)
        a1 = _pair(neta, x)
        fresh = _net(5)
        fresh.load_state_dict(copy.deepcopy(neta.state_dict()))
        assert torch.equal(a1, _pair(fresh, x))
        assert not torch.equal(a1, a0)
        neta.layers[0].conv.bias.add_(0.01)
        fresh.load_state_dict(copy.deepcopy(neta.state_dict()))
        assert torch.equal(_pair(neta, x), _pair(fresh, x))
    _no_timeouts()


# (N, H, W, height of the extended input whose last tile row is full): vr = OH mod 8 = 1, 2, 3, 4, 5, 7 on one tile row
# and a bit; c2's own vr = 2 (OH = 250 and 258); vr = 2 and 4 on runs of about six tiles that cross several short tiles
DEAD_ROW_SHAPES = ([(3, h, 60, 30) for h in (15, 16, 17, 18, 19, 21)] + [(2, 256, 40, 262), (2, 264, 40, 270)]
                   + [(40, 16, 300, 22), (40, 18, 300, 22)])


@pytest.mark.parametrize("shape", DEAD_ROW_SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_short_last_tile_equals_the_full_one(shape):
    """The rows a short last tile stores are the rows the same tile stores when the input goes on downwards and the tile
    is full.  Both inputs are declared |x| <= 1, so both split at one scale."""
    n, h, w, hx = shape
    assert (hx - 6) % 8 == 0
    net = _net()
    torch.manual_seed(9)
    xl = torch.rand(n, 3, hx, w, device="cuda")
    xs = xl[:, :, :h, :].contiguous()
    with torch.no_grad():
        full = _pair(net, ops.declare_absmax(xl, 1.0))
        short = _pair(net, ops.declare_absmax(xs, 1.0))
    assert short.shape[2] == h - 6
    assert torch.equal(short, full[:, :, :h - 6, :])
    _no_timeouts()


@pytest.mark.parametrize("shape", [(2, 16, 60), (2, 86, 486)])
def test_accuracy_stays_where_it_was(shape):
    """test_espcn_pair_walk_gpu.test_run_boundaries_match_two_launches_and_fp64's comparison and bounds, with the maximum
    measured inside the launch."""
    n, h, w = shape
    net = _net()
    torch.manual_seed(4)
    x = torch.rand(n, 3, h, w, device="cuda")
    xu = x.clone()
    with torch.no_grad():
        y2 = net.layers[1](net.layers[0](x))
        assert getattr(xu, "_srk_amax", None) is None
        y1 = _pair(net, xu)
    assert y1.shape == y2.shape
    ref = _ref64(net, x)
    e1, e2 = _err(y1, ref), _err(y2, ref)
    print("shape %s  pair max %.3e rms %.3e   two launches max %.3e rms %.3e   pair - two %.3e"
          % (shape, e1[0], e1[1], e2[0], e2[1], (y1 - y2).abs().max().item() / y2.abs().max().item()))
    assert e1[0] <= 1.5 * e2[0] + 1e-7 and e1[1] <= 1.5 * e2[1] + 1e-8, (e1, e2)
    assert (y1 - y2).abs().max().item() <= 1e-5 * y2.abs().max().item()
    _no_timeouts()
