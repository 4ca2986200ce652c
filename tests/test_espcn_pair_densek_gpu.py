"""k_espcn_pair's first layer with its K packed densely (csrc/conv_pair.hip: 8 MFMA steps, every product of the f16x3
sum in a K slot of its own).  The second conv is a selector -- weight 1 at the centre tap from one first-layer channel,
bias 0 -- so the kernel's output shows 32 first-layer channels directly; two selectors cover all 64.  The bars are the
suite's: against the two-launch path (k_conv_rowsr + k_conv_bfr) and against fp64."""
import functools

import pytest
import torch

from pytorch_super_resolution_model_collection_amd import _lib, models, ops

pytestmark = pytest.mark.gpu

SHAPE = (8, 3, 150, 120)    # 1152 tiles: several per block down a column, fresh tops, short last tiles
SMALL = (2, 3, 37, 53)
SELECTORS = (0, 32)
TAP_VALUES = (0.7, 0.3, 1.1)   # each leaves an fp16 residual of at least 2^-13 relative (checked below)


def _select(net, first):
    """layers[1]: output channel o = first-layer channel first + o, as is."""
    c2 = net.layers[1].conv
    with torch.no_grad():
        c2.weight.zero_()
        c2.bias.zero_()
        for o in range(32):
            c2.weight[o, first + o, 1, 1] = 1.0
    return net


def _random_net(first):
    torch.manual_seed(0)
    net = models.ESPCNNet(3, 64, 4).cuda()
    net.weight_init()
    with torch.no_grad():
        net.layers[0].conv.bias.uniform_(-0.05, 0.05)
    return _select(net, first).eval()


def _tap_net(first, shift):
    """One non-zero weight per first-layer channel: channel c has tap (c + shift) mod 75 of the 75 (ci, dy, dx)."""
    net = models.ESPCNNet(3, 64, 4).cuda()
    c1 = net.layers[0].conv
    with torch.no_grad():
        c1.weight.zero_()
        c1.bias.zero_()
        flat = c1.weight.view(64, 75)
        for c in range(64):
            flat[c, (c + shift) % 75] = TAP_VALUES[c % len(TAP_VALUES)]
    return _select(net, first).eval()


@functools.lru_cache(maxsize=None)
def _input(shape, seed):
    torch.manual_seed(seed)
    return torch.rand(shape, device="cuda")


def _ref64(net, x):
    c1, c2 = net.layers[0].conv, net.layers[1].conv
    y = torch.relu(torch.nn.functional.conv2d(x.double(), c1.weight.double(), c1.bias.double()))
    return torch.relu(torch.nn.functional.conv2d(y, c2.weight.double(), c2.bias.double()))


def _err(y, ref):
    d = (y.double() - ref).abs()
    scale = ref.abs().max().item()
    return d.max().item() / scale, d.pow(2).mean().sqrt().item() / scale


def _pair(net, x):
    y = ops.espcn_pair(x, net.layers[0], net.layers[1], force=True)
    assert y is not None
    assert _lib.load().srk_last_kernel_name().decode() == "k_espcn_pair"
    return y


def _check(net, x, what):
    assert _lib.load().srk_ring_timeouts(1) >= 0
    with torch.no_grad():
        y2 = net.layers[1](net.layers[0](x))
        y1 = _pair(net, x)
    assert y1.shape == y2.shape
    ref = _ref64(net, x)
    scale = ref.abs().max().item()
    e1, e2 = _err(y1, ref), _err(y2, ref)
    diff = (y1 - y2).abs().max().item()
    print("%s: pair max %.3e rms %.3e   two launches max %.3e rms %.3e   pair - two %.3e of max|ref|"
          % (what, e1[0], e1[1], e2[0], e2[1], diff / scale))
    assert torch.isfinite(y1).all()
    assert diff <= 1e-5 * scale
    assert e1[0] <= 1.5 * e2[0] + 1e-7 and e1[1] <= 1.5 * e2[1] + 1e-8, (e1, e2)
    torch.cuda.synchronize()
    assert _lib.load().srk_ring_timeouts(1) == 0


def test_tap_values_leave_a_residual():
    for v in TAP_VALUES:
        w = torch.tensor(v, dtype=torch.float32)
        assert abs((w - w.to(torch.float16).float()).item()) >= 2.0 ** -13 * v


def test_two_shifts_reach_every_tap():
    assert {(c + s) % 75 for s in (0, 37) for c in range(64)} == set(range(75))


@pytest.mark.parametrize("first", SELECTORS)
@pytest.mark.parametrize("shift", [0, 37])
def test_every_tap_is_wired(shift, first):
    """A dropped or mis-addressed K slot misses its term (w_h x_h, w_h x_m or w_m x_h) of every element of that channel:
    at least about 2.4e-4 of the element for the smallest, three orders above the bars."""
    _check(_tap_net(first, shift), _input(SHAPE, 11), "taps shift %d channels %d.." % (shift, first))


@pytest.mark.parametrize("first", SELECTORS)
@pytest.mark.parametrize("shape", [SHAPE, SMALL], ids=lambda s: "x".join(map(str, s)))
def test_random_filter(shape, first):
    _check(_random_net(first), _input(shape, 12), "random filter %s channels %d.." % (shape, first))


@pytest.mark.parametrize("shape", [(2, 3, 86, 486), (3, 3, 47, 61)], ids=lambda s: "x".join(map(str, s)))
def test_pad_slots_are_inert(shape):
    """The in-launch max|x| path uses the staging region as scratch before the first tile; slots of the staged tile that
    no pixel writes meet zero weights and must not show: the same input with a declared maximum gives the same bits."""
    torch.manual_seed(0)
    net = models.ESPCNNet(3, 64, 4).cuda()
    net.weight_init()
    net.eval()
    x = _input(shape, 13).clone()
    assert getattr(x, "_srk_amax", None) is None
    with torch.no_grad():
        a = _pair(net, x)                                                    # measures max|x| in the launch
        b = _pair(net, ops.declare_absmax(x.clone(), x.abs().max().item()))
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    assert _lib.load().srk_ring_timeouts(1) == 0
