"""The training degradations without a GPU: the Philox known answers, the host twins of the library (the noise normals and
the blur tables, the code the kernels compile) against the fp64 restatement in degrade_ref.py, the argument checks that
come before any launch, the draws from Python's `random`, the command line, and the guard that lets the GPU tests demand
byte equality: no value of the case table rounds within 1e-7 of a boundary."""
import ctypes
import math
import random

import numpy as np
import pytest

import __graft_entry__
import degrade_ref as R

PD = ctypes.POINTER(ctypes.c_double)
PU = ctypes.POINTER(ctypes.c_uint32)
INVALID = -1   # SRK_ERR_INVALID (= SRK_ERR_BAD_ARG, include/srk.h)

# Philox4x32-10 known answers (counter, key, output), as Random123's kat_vectors lists them
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def host_normals(lib, seed, first, n):
    z = np.full(n, np.nan)
    assert lib.srk_noise_normals_host(seed, first, n, z.ctypes.data_as(PD)) == 0, lib.srk_last_error_string()
    return z


def host_weights(lib, s1, s2, theta, K):
    w = np.full((K, K), np.nan)
    assert lib.srk_blur_weights_host(s1, s2, theta, K, w.ctypes.data_as(PD)) == 0, lib.srk_last_error_string()
    return w


def words(text):
    return [int(v, 16) for v in text.split()]


def test_philox_known_answers_mirror():
    for counter, key, want in KAT:
        assert [int(v) for v in R.philox4x32_10(counter, key)] == words(want)


def test_philox_known_answers_library(lib):
    """The generator the noise kernel compiles (csrc/degrade_common.h), through its host entry point."""
    for counter, key, want in KAT:
        out = (ctypes.c_uint32 * 4)()
        assert lib.srk_philox4x32_10_host((ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), out) == 0
        assert list(out) == words(want)
    # ... and through srk_noise_normals_host where its counters reach: seed 0, group 0 is the first vector.  Box-Muller
    # inverted: u(x0) = exp(-(n0^2 + n1^2) / 2), u(x1) = atan2(n1, n0) / 2 pi; a word is recovered to ~1e-5 of a unit.
    z = host_normals(lib, 0, 0, 4)
    x = words(KAT[0][2])
    for h in range(2):
        u0 = math.exp(-0.5 * (z[2 * h] ** 2 + z[2 * h + 1] ** 2))
        u1 = (math.atan2(z[2 * h + 1], z[2 * h]) / (2 * math.pi)) % 1.0
        assert abs(u0 * 2.0 ** 32 - 0.5 - x[2 * h]) < 1e-3 and abs(u1 * 2.0 ** 32 - 0.5 - x[2 * h + 1]) < 1e-3


@pytest.mark.parametrize("seed,first,n", [
    (0, 0, 64), (1, 0, 1), (0x0123456789abcdef, 0, 4099),
    (0xfedcba9876543210, 1, 7), (5, 2, 9), (5, 3, 1), (5, 7, 6),              # first elements that are no multiple of 4
    (0xffffffffffffffff, (1 << 34) + 1, 23), (3, (1 << 40) - 2, 11)])          # q >= 2^32: the counter's high word
def test_normals_host_matches_mirror(lib, seed, first, n):
    """Within 1e-14 absolute: both sides are fp64 and may differ by what their libm's log, sqrt, sin and cos round."""
    got, want = host_normals(lib, seed, first, n), R.normals(seed, first, n)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-14
    if first % 4 and n > 1:   # the lane is the element's, not the position's in the call
        assert np.array_equal(got[1:], host_normals(lib, seed, first + 1, n - 1))
    if first >> 34:           # the high word matters: the low words alone give other numbers
        assert np.abs(got - host_normals(lib, seed, first & ((1 << 34) - 1), n)).max() > 1e-3


def test_normals_are_normal(lib):
    z = host_normals(lib, 0x9e3779b97f4a7c15, 0, 1 << 16)
    n = z.size
    assert abs(z.mean()) < 5 / math.sqrt(n) and abs(z.std() - 1) < 5 / math.sqrt(2 * n)
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 5 / math.sqrt(n)


def _table_args():
    rs = random.Random(7)
    args = [(0.2, 0.2, 0.0), (4.0, 4.0, 1.0), (4.0, 0.2, math.pi / 4), (0.2, 4.0, 3.0), (1.0, 2.0, math.pi / 2)]
    args += [(rs.uniform(0.2, 4.0), rs.uniform(0.2, 4.0), rs.uniform(0, math.pi)) for _ in range(40)]
    return args


def test_blur_weights_host_matches_mirror(lib, pkg):
    sizes = set()
    for s1, s2, th in _table_args():
        K = R.kernel_size(s1, s2)
        assert K == pkg.data.blur_kernel_size(s1, s2) and K % 2 == 1 and 3 <= K <= 21
        sizes.add(K)
        w, want = host_weights(lib, s1, s2, th, K), R.blur_weights(s1, s2, th, K)
        assert np.abs(w - want).max() <= 1e-15
        assert abs(math.fsum(w.ravel()) - 1.0) <= 4e-16          # the exact sum of the fp64 table
        assert np.array_equal(w, w[::-1, ::-1])                   # w[i][j] == w[K-1-i][K-1-j], exactly
        assert np.abs(w - host_weights(lib, s1, s2, th + math.pi, K)).max() <= 1e-15
        assert w.min() >= 0 and np.unravel_index(w.argmax(), w.shape) == (K // 2, K // 2)
        assert np.array_equal(pkg.data.blur_weights(s1, s2, th), w)
    assert {3, 21} <= sizes and len(sizes) >= 6
    assert R.kernel_size(0.2, 0.2) == 3 and R.kernel_size(1.0, 0.3) == 7 and R.kernel_size(3.34, 1.0) == 21 \
        and R.kernel_size(4.0, 4.0) == 21
    # an isotropic table does not depend on the angle; an anisotropic one follows it: sigma 3 along x at theta 0
    assert np.abs(host_weights(lib, 1.5, 1.5, 0.3, 11) - host_weights(lib, 1.5, 1.5, 1.9, 11)).max() <= 1e-15
    w = host_weights(lib, 3.0, 0.5, 0.0, 19)
    assert w[9, 15] > 0.1 * w[9, 9] and w[15, 9] < 1e-12 * w[9, 9]
    for bad in ((1.0, 1.0, 0.0, 4), (1.0, 1.0, 0.0, 23), (0.0, 1.0, 0.0, 5), (1.0, -1.0, 0.0, 5)):
        assert lib.srk_blur_weights_host(*bad, np.zeros(23 * 23).ctypes.data_as(PD)) == INVALID
    assert lib.srk_blur_weights_host(1.0, 1.0, 0.0, 5, None) == INVALID


def test_arguments_are_checked_before_any_launch(lib):
    """No device is touched: the pointers are never dereferenced, nothing is launched (this test runs without a GPU)."""
    buf = np.zeros(64 * 64, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    blur = lambda x, y, w, ppp, B, H, W, K: lib.srk_blur_u8(x, y, w, ppp, B, H, W, K, None)
    assert blur(p, p, p, 3, 1, 32, 32, 4) == INVALID      # K even
    assert blur(p, p, p, 3, 1, 32, 32, 23) == INVALID     # K = 23
    assert blur(p, p, p, 3, 1, 32, 32, 1) == INVALID      # K = 1
    assert blur(p, p, p, 3, 1, 10, 32, 21) == INVALID     # H = K / 2
    assert blur(p, p, p, 3, 1, 32, 10, 21) == INVALID     # W = K / 2
    assert blur(p, p, p, 3, 1, 3, 32, 7) == INVALID
    assert b"reflect" in lib.srk_last_error_string()
    assert blur(None, p, p, 3, 1, 32, 32, 5) == INVALID and blur(p, None, p, 3, 1, 32, 32, 5) == INVALID \
        and blur(p, p, None, 3, 1, 32, 32, 5) == INVALID
    assert blur(p, p, p, 0, 1, 32, 32, 5) == INVALID and blur(p, p, p, 3, 0, 32, 32, 5) == INVALID
    noise = lambda x, y, s, B, n: lib.srk_noise_u8(x, y, s, 1, B, n, None)
    assert noise(None, p, p, 1, 16) == INVALID and noise(p, None, p, 1, 16) == INVALID and noise(p, p, None, 1, 16) == INVALID
    assert noise(p, p, p, 0, 16) == INVALID and noise(p, p, p, 1, 0) == INVALID
    assert lib.srk_noise_normals_host(1, 0, 4, None) == INVALID and lib.srk_philox4x32_10_host(None, None, None) == INVALID
    assert lib.srk_version() == 600


def test_ops_raise_on_cpu_tensors(pkg):
    import torch
    x = torch.zeros((1, 1, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        pkg.ops.blur_u8(x, torch.zeros((1, 3, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        pkg.ops.noise_u8(x, torch.zeros(1, dtype=torch.float64), 1)


# -- draws -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(blur_prob=0.5), dict(noise_sigma=(0.0, 0.0)), dict(blur_prob=0.0),
                                dict(blur_prob=0.3, blur_sigma=(0.5, 1.0), noise_sigma=(2.0, 2.0))])
def test_draw_consumes_random_in_the_documented_order(pkg, kw):
    deg = pkg.data.Degradation(**kw)
    lo, hi = deg.blur_sigma
    nlo, nhi = deg.noise_sigma
    for seed, batch in ((0, 1), (1, 2), (2, 16)):
        random.seed(seed)
        w, sigma, nseed = deg.draw(batch)
        after = random.getstate()
        random.seed(seed)                       # the replay, by hand
        params = []
        for _ in range(batch):
            blurred = random.random() < deg.blur_prob
            params.append((random.uniform(lo, hi), random.uniform(lo, hi), random.uniform(0, math.pi)) if blurred else None)
            params.append(random.uniform(nlo, nhi) if nhi > 0 else 0.0)
        want_seed = random.getrandbits(64) if nhi > 0 else 0
        assert random.getstate() == after and nseed == want_seed
        assert np.array_equal(sigma, np.array(params[1::2]))
        K = max([R.kernel_size(p[0], p[1]) for p in params[0::2] if p] + [3])
        assert w.shape == (batch, K, K) and w.dtype == np.float64
        for b, p in enumerate(params[0::2]):
            want = R.centred(R.blur_weights(*p, R.kernel_size(p[0], p[1])) if p else R.delta(3), K)
            assert np.abs(w[b] - want).max() <= 1e-15 and (p is not None or np.array_equal(w[b], want))
        random.seed(seed)                       # the mirror's own draw agrees
        mw, msigma, mseed = R.draw(batch, deg.blur_prob, deg.blur_sigma, deg.noise_sigma)
        assert random.getstate() == after and mseed == nseed and np.array_equal(msigma, sigma) and mw.shape == w.shape


def test_degradation_rejects_bad_ranges(pkg):
    D = pkg.data.Degradation
    for kw in (dict(blur_sigma=(2.0, 1.0)), dict(blur_sigma=(0.0, 1.0)), dict(blur_sigma=(-1.0, 1.0)),
               dict(noise_sigma=(-1.0, 2.0)), dict(noise_sigma=(3.0, 2.0)), dict(blur_prob=1.5), dict(blur_prob=-0.1)):
        with pytest.raises(ValueError):
            D(**kw)
    d = D()
    assert d.blur_prob == 1.0 and d.blur_sigma == (0.2, 4.0) and d.noise_sigma == (0.0, 10.0)
    with pytest.raises(ValueError):
        pkg.data.TestDatasetFromFolder(".", degrade=(1.0, 0.0, 0.0, 1.0))


class _FakeDevice(object):
    """Stands in for data._Device where no GPU is: records the calls of a finish() and hands back host tensors."""

    def __init__(self):
        self.calls = []

    def resize(self, x, strides, planes, h, w, oh, ow, out_float):
        import torch
        self.calls.append("resize_f32" if out_float else "resize_u8")
        return torch.zeros((planes, oh, ow), dtype=torch.float32 if out_float else torch.uint8)

    def bicubic_of_lr(self, lr, oh, ow):
        import torch
        self.calls.append("bicubic_of_lr")
        return torch.zeros(tuple(lr.shape[:2]) + (oh, ow))

    def upload_f64(self, values):
        import torch
        self.calls.append("upload_f64")
        return torch.from_numpy(np.array(values, np.float64))

    def blur(self, x, weights, planes_per_patch, b, h, w):
        self.calls.append("blur")
        return x

    def noise(self, x, sigma, seed, b):
        self.calls.append("noise")
        return x.float()


def test_finish_draws_only_when_degrading(pkg, tmp_path):
    """degrade=None: draw + finish leave `random` where they left it before this feature -- finish makes no draw, and runs
    the two resizes and the bicubic image it always ran.  With a Degradation the draws of its draw() follow the patch's,
    and the launches are blur, the 8-bit shrink and the noise."""
    import torch
    (tmp_path / "train").mkdir()
    patches = torch.zeros((2, 3, 32, 32), dtype=torch.uint8)
    ds = pkg.data.TrainDatasetFromFolder([str(tmp_path / "train")], crop_size=32, scale_factor=4)
    assert ds.degrade is None
    ds._dev = _FakeDevice()
    random.seed(3)
    ds.draw(97, 61)
    want = random.getstate()
    lr, hr, bc = ds.finish(patches)
    assert random.getstate() == want and ds._dev.calls == ["resize_f32", "resize_f32", "bicubic_of_lr"]
    assert lr.shape == (2, 3, 8, 8) and hr.shape == (2, 3, 32, 32) and bc.shape == hr.shape

    deg = pkg.data.Degradation(blur_prob=1.0, noise_sigma=(1.0, 5.0))
    ds = pkg.data.get_training_set(str(tmp_path), ["train"], 32, 4, degrade=deg)
    assert ds.degrade is deg
    ds._dev = _FakeDevice()
    random.seed(3)
    ds.draw(97, 61)
    ds.finish(patches)
    got = random.getstate()
    random.seed(3)
    ds.draw(97, 61)
    deg.draw(2)
    assert random.getstate() == got and got != want
    assert ds._dev.calls == ["resize_f32", "upload_f64", "blur", "resize_u8", "noise", "bicubic_of_lr"]
    # no blur drawn and no noise asked for: the clean shrink's launches, but the blur's coin is still tossed
    ds.degrade = pkg.data.Degradation(blur_prob=0.0, noise_sigma=(0.0, 0.0))
    ds._dev = _FakeDevice()
    random.seed(3)
    ds.finish(patches)
    after = random.getstate()
    random.seed(3)
    random.random(), random.random()
    assert random.getstate() == after and ds._dev.calls == ["resize_f32", "resize_f32", "bicubic_of_lr"]


# -- command line ------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    import main as cli
    base = ["--model_name", "EDSR", "--save_dir", str(tmp_path / "out")]
    a = cli.parse_args(base)
    assert a.degrade is False and a.blur_sigma == (0.2, 4.0) and a.blur_prob == 1.0 and a.noise_sigma == (0.0, 10.0) \
        and a.degrade_test is None
    a = cli.parse_args(base + ["--degrade", "--blur_sigma", "0.5,2", "--blur_prob", "0.8", "--noise_sigma", "1,25",
                               "--degrade_test", "1.2,2.0,30,5"])
    assert a.degrade and a.blur_sigma == (0.5, 2.0) and a.blur_prob == 0.8 and a.noise_sigma == (1.0, 25.0) \
        and a.degrade_test == (1.2, 2.0, 30.0, 5.0)
    assert cli.parse_args(base + ["--noise_sigma", "0,0"]).noise_sigma == (0.0, 0.0)
    for bad in (["--blur_sigma", "2,1"], ["--blur_sigma", "0,1"], ["--blur_sigma", "-1,1"], ["--blur_sigma", "1"],
                ["--blur_sigma", "a,b"], ["--blur_sigma", "nan,1"], ["--noise_sigma", "-1,2"], ["--noise_sigma", "3,2"],
                ["--noise_sigma", "1,2,3"], ["--blur_prob", "1.5"], ["--blur_prob", "x"],
                ["--degrade_test", "0,1,0,1"], ["--degrade_test", "1,1,0,-1"], ["--degrade_test", "1,1,0"],
                ["--degrade", "--synthetic"], ["--degrade_test", "1,1,0,1", "--synthetic"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert "--degrade" in capsys.readouterr().err


def test_trainer_refuses_degrade_with_synthetic(pkg):
    """The ValueError behind the argument error, for callers that build the arguments themselves: it names the flag and
    comes before the trainer asks for a GPU."""
    from types import SimpleNamespace
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    for flag, value in (("degrade", True), ("degrade_test", (1.0, 1.0, 0.0, 1.0))):
        args = SimpleNamespace(model_name="EDSR", synthetic=True, **{flag: value})
        with pytest.raises(ValueError, match=flag):
            TRAINERS["EDSR"](args)


# -- the guard ---------------------------------------------------------------------------------------------------------
GUARD = 1e-7


@pytest.mark.parametrize("name", [c[0] for c in R.BLUR_CASES])
def test_guard_blur_cases(name):
    """A condition on the case table, not a tolerance: the device's fp64 sum of at most 441 taps of values <= 255 is
    within ~3e-11 of the mirror's, so a value 1e-7 from every rounding boundary rounds the same on both sides and the GPU
    test may demand zero mismatches.  If an entry fails here, change its seed."""
    p, w = R.blur_case(name)
    assert R.boundary_distance(R.blur_pre(p, w)) >= GUARD
    assert np.abs(w.sum(axis=(1, 2)) - 1).max() < 1e-14


@pytest.mark.parametrize("name", [c[0] for c in R.NOISE_CASES])
def test_guard_noise_cases(name):
    x, sigma, seed = R.noise_case(name)
    assert R.boundary_distance(R.noise_pre(x, sigma, seed)) >= GUARD


def test_guard_identities_and_statistics():
    K = 21
    w = R.tables(31, 2, K, ['full'])
    for v in (0, 255):
        p = np.full((2, 1, 24, 24), v, np.uint8)
        assert R.boundary_distance(R.blur_pre(p, w)) >= GUARD and (R.blur(p, w) == v).all()
    for v in (0, 255, 128):
        x = np.full((16, 3, 32, 32), v, np.uint8)
        assert R.boundary_distance(R.noise_pre(x, np.full(16, 25.0 if v != 128 else 10.0), R.STAT_SEED)) >= GUARD


@pytest.mark.parametrize("is_gray", [False, True])
def test_guard_end_to_end(tmp_path, is_gray):
    folder = R.make_folder(str(tmp_path / "train"))
    batches = R.replay_batches(folder, 2, is_gray)
    for b in batches:
        assert b["blur_guard"] >= GUARD and b["noise_guard"] >= GUARD
    assert 0 < sum(b["blurred"] for b in batches) < 2 * R.E2E["batch"]     # blurred and unblurred patches both occur
    from PIL import Image
    for i in range(2):
        hwc = np.asarray(Image.open(folder + "/img_%02d.png" % i).convert("RGB").convert("YCbCr" if is_gray else "RGB"))
        s1, s2, th, ns = R.TEST_DEGRADE
        planes = np.ascontiguousarray(hwc.transpose(2, 0, 1))[None]
        w = R.blur_weights(s1, s2, th, R.kernel_size(s1, s2))[None]
        assert R.boundary_distance(R.blur_pre(planes, w)) >= GUARD
        sf = R.E2E["scale_factor"]
        q = R.pil_resize(R.blur(planes, w), hwc.shape[0] // sf, hwc.shape[1] // sf)
        assert R.boundary_distance(R.noise_pre(q, [ns], i)) >= GUARD
