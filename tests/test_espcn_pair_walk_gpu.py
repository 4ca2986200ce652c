"""The fused ESPCN pair kernel walks tile columns and takes the two shared halo rows of the intermediate from the tile
above (csrc/conv_pair.hip): a reused row must be the number a tile computing it itself would get, wherever a block's run
of tiles starts or ends."""
import pytest
import torch

from pytorch_super_resolution_model_collection_amd import _lib, models, ops

pytestmark = pytest.mark.gpu


def _net(seed=0):
    torch.manual_seed(seed)
    net = models.ESPCNNet(3, 64, 4).cuda()
    net.weight_init()
    with torch.no_grad():   # non-zero biases: the bound of the intermediate sees them
        for b in (net.layers[0].conv.bias, net.layers[1].conv.bias):
            b.uniform_(-0.05, 0.05)
    return net.eval()


def _pair(net, x):
    y = ops.espcn_pair(x, net.layers[0], net.layers[1], force=True)
    assert y is not None
    assert _lib.load().srk_last_kernel_name().decode() == "k_espcn_pair"
    return y


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


@pytest.mark.parametrize("crop", [("rows", 8), ("rows", 24), ("cols", 16)])
def test_shift_invariance_is_bit_exact(crop):
    """Rows that one run takes from the tile above, the other computes itself: both inputs are declared |x| <= 1, so both
    runs split at one scale and every output must be the same bits."""
    axis, k = crop
    net = _net()
    torch.manual_seed(3)
    x = torch.rand(8, 3, 150, 120, device="cuda")
    xc = (x[:, :, k:, :] if axis == "rows" else x[:, :, :, k:]).contiguous()
    assert _lib.load().srk_ring_timeouts(1) >= 0
    with torch.no_grad():
        a = _pair(net, ops.declare_absmax(x, 1.0))
        b = _pair(net, ops.declare_absmax(xc, 1.0))
    ac = a[:, :, k:, :] if axis == "rows" else a[:, :, :, k:]
    assert ac.shape == b.shape
    assert torch.equal(ac, b)
    _no_timeouts()


# output heights with OH mod 8 in {0, 1, 7}; a single tile row (H = 7 .. 14); one tile column (W <= 22); N = 1; tile
# columns that do not divide among the CUs, so that runs start and end inside columns
BOUNDARY_SHAPES = [(2, 46, 60), (2, 47, 60), (2, 53, 60), (4, 7, 200), (3, 10, 90), (6, 14, 300), (5, 120, 22), (9, 90, 7),
                   (1, 200, 150), (1, 75, 19), (5, 100, 257), (3, 263, 41), (7, 9, 300)]


@pytest.mark.parametrize("shape", BOUNDARY_SHAPES)
def test_run_boundaries_match_two_launches_and_fp64(shape):
    n, h, w = shape
    net = _net()
    torch.manual_seed(4)
    x = torch.rand(n, 3, h, w, device="cuda")
    assert _lib.load().srk_ring_timeouts(1) >= 0
    with torch.no_grad():
        y2 = net.layers[1](net.layers[0](x))
        y1 = _pair(net, x)
    assert y1.shape == y2.shape
    ref = _ref64(net, x)
    e1, e2 = _err(y1, ref), _err(y2, ref)
    print("shape %s  pair max %.3e rms %.3e   two launches max %.3e rms %.3e   pair - two %.3e"
          % (shape, e1[0], e1[1], e2[0], e2[1], (y1 - y2).abs().max().item() / y2.abs().max().item()))
    assert e1[0] <= 1.5 * e2[0] + 1e-7 and e1[1] <= 1.5 * e2[1] + 1e-8, (e1, e2)
    assert (y1 - y2).abs().max().item() <= 1e-5 * y2.abs().max().item()
    _no_timeouts()


@pytest.mark.parametrize("shape", [(64, 256, 256), (5, 100, 257)])
def test_same_call_three_times_is_bit_exact(shape):
    n, h, w = shape
    net = _net()
    torch.manual_seed(5)
    x = torch.rand(n, 3, h, w, device="cuda")
    with torch.no_grad():
        a, b, c = _pair(net, x), _pair(net, x), _pair(net, x)
    assert torch.equal(a, b) and torch.equal(a, c)
    _no_timeouts()
