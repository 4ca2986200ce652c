"""The JPEG stage of the training degradations without a GPU: the integer restatement in jpeg_ref.py against Pillow's own
save / open on the whole case table (zero differing bytes, nothing masked), the library's host twin (the very bodies the
kernel compiles, csrc/jpeg_common.h) against the restatement, the quantisation tables, the argument checks that come
before any launch, the draws from Python's `random`, the launches of a finish(), and the command line."""
import ctypes
import functools
import random

import numpy as np
import pytest

import __graft_entry__
import degrade_ref as R
import jpeg_ref as J

INVALID = -1   # SRK_ERR_INVALID (= SRK_ERR_BAD_ARG, include/srk.h)


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@functools.lru_cache(maxsize=None)
def want(name):
    x, q, sub, color = J.case(name)
    return x, q, sub, color, J.jpeg_one(x, q, sub, color)


def mismatch(name, got, ref):
    bad = got != ref
    return "%s: %d of %d bytes differ, first at %s: got %d want %d" % (
        name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0]) if bad.any() else ""


def host_jpeg(lib, x, quality, sub, color):
    x = np.ascontiguousarray(x)
    y = np.full_like(x, 77)
    B, C, H, W = x.shape
    q = (ctypes.c_int * B)(*[int(v) for v in quality])
    rc = lib.srk_jpeg_u8_host(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data), q, C, B, H, W, sub, color)
    assert rc == 0, lib.srk_last_error_string()
    return y


def test_case_table_covers_what_it_must():
    sizes = {(c[3][1], c[3][2]) for c in J.CASES}
    assert {(1, 1), (7, 7), (8, 8), (16, 16), (17, 9), (23, 39), (32, 32), (33, 31), (34, 18), (40, 40), (70, 90)} <= sizes
    for size in sizes:
        combos = {(c[3][0], c[5], c[6]) for c in J.CASES if (c[3][1], c[3][2]) == size and c[1] != "checker"}
        assert combos == {(3, 1, 1), (3, 0, 1), (3, 1, 0), (3, 0, 0), (1, 0, 0)}, size
    assert {c[1] for c in J.CASES} == {"noise", "smooth", "checker"}
    assert {5, 100} <= {c[4] for c in J.CASES} and len(set(J.NAMES)) == len(J.NAMES)


@pytest.mark.parametrize("name", J.NAMES)
def test_restatement_equals_pillow(name):
    """Image.save(format='JPEG', quality=q, subsampling=...) then Image.open: RGB, YCbCr read back without the colour tail,
    and L.  Also the guard of the definition's clamp: no case, the 0 / 255 checkerboard at quality 5 included, reaches
    values where libjpeg would wrap instead."""
    if not J.turbo():
        pytest.skip("Pillow is not built on libjpeg-turbo: its bytes are not the ones the definition restates")
    x, q, sub, color, ref = want(name)
    got = J.pillow_one(x, q, sub, color)
    assert got.shape == ref.shape and not mismatch(name, ref, got), mismatch(name, ref, got)


@pytest.mark.parametrize("name", J.NAMES)
def test_host_twin_equals_restatement(lib, name):
    x, q, sub, color, ref = want(name)
    got = host_jpeg(lib, x[None], [q], sub, color)[0]
    assert not mismatch(name, got, ref), mismatch(name, got, ref)


def test_host_twin_batch_and_quality_zero(lib):
    x, q = J.batch_case()
    for sub in (1, 0):
        got, ref = host_jpeg(lib, x, q, sub, 1), J.jpeg(x, q, sub, 1)
        assert not mismatch("batch", got, ref), mismatch("batch", got, ref)
        assert np.array_equal(got[0], x[0]) and all(not np.array_equal(got[b], x[b]) for b in range(1, len(q)))
    for v in (0, 128, 255):      # a constant plane has no AC energy and its DC survives every table
        for C, color in ((1, 0), (3, 0), (3, 1)):
            p = np.full((1, C, 23, 39), v, np.uint8)
            assert (host_jpeg(lib, p, [75], 1, color) == v).all() and (J.jpeg(p, 75, 1, color) == v).all()


def test_quant_tables(lib):
    def table(q, chroma):
        out = (ctypes.c_int * 64)()
        assert lib.srk_jpeg_quant_table_host(q, chroma, out) == 0
        return np.array(out, np.int64).reshape(8, 8)
    for q in (1, 2, 25, 49, 50, 51, 75, 99, 100):
        for chroma in (0, 1):
            assert np.array_equal(table(q, chroma), J.quant_table(q, chroma)), (q, chroma)
    for chroma in (0, 1):
        assert (table(100, chroma) == 1).all()
        assert np.array_equal(table(0, chroma), table(1, chroma)) and np.array_equal(table(-7, chroma), table(1, chroma))
        assert np.array_equal(table(101, chroma), table(100, chroma)) and np.array_equal(table(1000, chroma), table(100, chroma))
    assert table(50, 0)[0, 0] == 16 and table(50, 1)[0, 0] == 17 and table(50, 0)[7, 7] == 99     # quality 50: Annex K itself
    assert table(1, 0).max() == 255 and table(25, 0)[0, 0] == 32 and table(75, 0)[0, 0] == 8
    assert lib.srk_jpeg_quant_table_host(50, 2, (ctypes.c_int * 64)()) == INVALID
    assert lib.srk_jpeg_quant_table_host(50, 0, None) == INVALID


def test_arguments_are_checked_before_any_launch(lib):
    """No device is touched: the pointers are never dereferenced, nothing is launched (this test runs without a GPU)."""
    buf = np.zeros(3 * 64 * 64 * 4, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    jpeg = lambda x, y, q, C, B, H, W, sub, color, flt=0: lib.srk_jpeg_u8(x, y, q, C, B, H, W, sub, color, flt, None)
    assert jpeg(None, p, p, 3, 1, 32, 32, 1, 1) == INVALID and jpeg(p, None, p, 3, 1, 32, 32, 1, 1) == INVALID \
        and jpeg(p, p, None, 3, 1, 32, 32, 1, 1) == INVALID
    assert b"null" in lib.srk_last_error_string()
    assert jpeg(p, p, p, 2, 1, 32, 32, 1, 0) == INVALID and jpeg(p, p, p, 4, 1, 32, 32, 0, 0) == INVALID \
        and jpeg(p, p, p, 0, 1, 32, 32, 0, 0) == INVALID
    assert jpeg(p, p, p, 1, 1, 32, 32, 0, 1) == INVALID           # colour needs three planes
    assert b"color" in lib.srk_last_error_string()
    assert jpeg(p, p, p, 3, 1, 32, 32, 2, 1) == INVALID and jpeg(p, p, p, 3, 1, 32, 32, -1, 1) == INVALID
    assert b"subsampling" in lib.srk_last_error_string()
    assert jpeg(p, p, p, 3, 0, 32, 32, 1, 1) == INVALID and jpeg(p, p, p, 3, 1, 0, 32, 1, 1) == INVALID \
        and jpeg(p, p, p, 3, 1, 32, -1, 1, 1) == INVALID and jpeg(p, p, p, 3, 1, 32, 0, 1, 1, 1) == INVALID
    q = (ctypes.c_int * 1)(50)
    host = lambda x, y, qq, C, B, H, W, sub, color: lib.srk_jpeg_u8_host(x, y, qq, C, B, H, W, sub, color)
    assert host(None, p, q, 3, 1, 8, 8, 1, 1) == INVALID and host(p, None, q, 3, 1, 8, 8, 1, 1) == INVALID \
        and host(p, p, None, 3, 1, 8, 8, 1, 1) == INVALID
    assert host(p, p, q, 2, 1, 8, 8, 1, 0) == INVALID and host(p, p, q, 1, 1, 8, 8, 0, 1) == INVALID \
        and host(p, p, q, 3, 1, 8, 8, 3, 1) == INVALID and host(p, p, q, 3, 1, 8, 0, 1, 1) == INVALID
    noise = lambda x, y, s, B, n: lib.srk_noise_u8_bytes(x, y, s, 1, B, n, None)
    assert noise(None, p, p, 1, 16) == INVALID and noise(p, None, p, 1, 16) == INVALID and noise(p, p, None, 1, 16) == INVALID
    assert noise(p, p, p, 0, 16) == INVALID and noise(p, p, p, 1, 0) == INVALID
    assert b"noise_u8_bytes" in lib.srk_last_error_string()
    assert lib.srk_version() == 600


def test_ops_raise_on_cpu_tensors_and_bad_arguments(pkg):
    import torch
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        pkg.ops.jpeg_u8(x, 50)
    with pytest.raises(RuntimeError, match="GPU"):
        pkg.ops.noise_u8_bytes(x, torch.zeros(1, dtype=torch.float64), 1)
    assert pkg.ops.jpeg_subsampling('4:2:0') == 1 == pkg.ops.jpeg_subsampling('420') \
        and pkg.ops.jpeg_subsampling('4:4:4') == 0 == pkg.ops.jpeg_subsampling('444')
    for bad in ('4:2:2', 422, None, [1]):
        with pytest.raises(ValueError, match="subsampling"):
            pkg.ops.jpeg_subsampling(bad)


# -- draws -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(jpeg_quality=(30, 95)), dict(jpeg_quality=(30, 95), jpeg_prob=0.5),
                                dict(jpeg_quality=(60, 60), jpeg_prob=0.0), dict(jpeg_quality=(1, 100), blur_prob=0.4),
                                dict(jpeg_quality=(40, 90), jpeg_prob=0.7, noise_sigma=(0.0, 0.0))])
def test_draw_jpeg_consumes_random_in_the_documented_order(pkg, kw):
    deg = pkg.data.Degradation(**kw)
    plain = pkg.data.Degradation(**{k: v for k, v in kw.items() if not k.startswith("jpeg")})
    lo, hi = deg.jpeg_quality
    for seed, batch in ((0, 1), (1, 2), (2, 16)):
        random.seed(seed)
        w, sigma, nseed = deg.draw(batch)
        mid = random.getstate()
        q = deg.draw_jpeg(batch)
        after = random.getstate()
        random.seed(seed)                       # draw() is untouched by the JPEG stage: the same draws, the same values
        pw, psigma, pseed = plain.draw(batch)
        assert random.getstate() == mid and np.array_equal(pw, w) and np.array_equal(psigma, sigma) and pseed == nseed
        assert plain.draw_jpeg(batch) is None and random.getstate() == mid     # off: nothing drawn
        want_q = []                             # the replay, by hand
        for _ in range(batch):
            want_q.append(random.randint(lo, hi) if random.random() < deg.jpeg_prob else 0)
        assert random.getstate() == after
        assert q.dtype == np.float64 and q.shape == (batch,) and q.tolist() == want_q
        random.setstate(mid)
        assert J.draw_jpeg(batch, deg.jpeg_quality, deg.jpeg_prob) == want_q and random.getstate() == after
        assert all(v == 0 or lo <= v <= hi for v in want_q)


def test_degradation_rejects_bad_jpeg_arguments(pkg, tmp_path):
    D = pkg.data.Degradation
    for kw in (dict(jpeg_quality=(0, 50)), dict(jpeg_quality=(50, 101)), dict(jpeg_quality=(60, 40)),
               dict(jpeg_quality=(30.5, 95)), dict(jpeg_quality=(30,)), dict(jpeg_quality=(30, 95), jpeg_prob=1.5),
               dict(jpeg_quality=(30, 95), jpeg_prob=-0.1), dict(jpeg_quality=(30, 95), jpeg_subsampling='4:2:2')):
        with pytest.raises(ValueError):
            D(**kw)
    d = D()
    assert d.jpeg_quality is None and d.jpeg_prob == 1.0 and d.jpeg_subsampling == 1
    assert D(jpeg_quality=(30, 95), jpeg_subsampling='4:4:4').jpeg_subsampling == 0
    for bad in (0, 101, 40.5):
        with pytest.raises(ValueError):
            pkg.data.TestDatasetFromFolder(str(tmp_path), jpeg=bad)
    with pytest.raises(ValueError):
        pkg.data.TestDatasetFromFolder(str(tmp_path), jpeg=40, jpeg_subsampling='411')
    ds = pkg.data.TestDatasetFromFolder(str(tmp_path), jpeg=40)
    assert ds.jpeg == 40 and ds.jpeg_subsampling == 1 and ds.degrade is None
    assert pkg.data.TestDatasetFromFolder(str(tmp_path)).jpeg is None


# -- launches ----------------------------------------------------------------------------------------------------------
class _FakeDevice(object):
    """Stands in for data._Device where no GPU is: records the calls of a finish() and hands back host tensors."""

    def __init__(self):
        self.calls, self.uploaded, self.jpeg_args = [], None, None

    def resize(self, x, strides, planes, h, w, oh, ow, out_float):
        import torch
        self.calls.append("resize_f32" if out_float else "resize_u8")
        return torch.zeros((planes, oh, ow), dtype=torch.float32 if out_float else torch.uint8)

    def bicubic_of_lr(self, lr, oh, ow):
        import torch
        assert lr.dtype == torch.float32
        self.calls.append("bicubic_of_lr")
        return torch.zeros(tuple(lr.shape[:2]) + (oh, ow))

    def upload_f64(self, values):
        import torch
        self.calls.append("upload_f64")
        self.uploaded = np.array(values, np.float64)
        return torch.from_numpy(self.uploaded.copy())

    def blur(self, x, weights, planes_per_patch, b, h, w):
        self.calls.append("blur")
        return x

    def noise(self, x, sigma, seed, b):
        self.calls.append("noise")
        return x.float()

    def noise_bytes(self, x, sigma, seed, b):
        import torch
        assert x.dtype == torch.uint8 and tuple(sigma.shape) == (b,)
        self.calls.append("noise_bytes")
        return x

    def jpeg(self, x, quality, subsampling, color):
        import torch
        assert x.dtype == torch.uint8 and quality.dtype == torch.float64 and tuple(quality.shape) == (x.shape[0],)
        self.calls.append("jpeg")
        self.jpeg_args = (quality.numpy().copy(), subsampling, color)
        return x.float()


def test_finish_launches_with_and_without_jpeg(pkg, tmp_path):
    """jpeg_quality=None: the launches and draws of a finish() are those from before this stage.  With it: blur, the 8-bit
    shrink, the noise as bytes, JPEG; the qualities ride behind the tables and the sigmas in the ONE parameter copy."""
    import torch
    (tmp_path / "train").mkdir()
    patches = torch.zeros((2, 3, 32, 32), dtype=torch.uint8)

    def run(deg, is_gray=False):
        ds = pkg.data.TrainDatasetFromFolder([str(tmp_path / "train")], crop_size=32, scale_factor=4, degrade=deg, is_gray=is_gray)
        ds._dev = _FakeDevice()
        random.seed(3)
        lr, hr, bc = ds.finish(patches)
        assert lr.shape == (2, 3, 8, 8) and lr.dtype == torch.float32 and hr.shape == (2, 3, 32, 32) and bc.shape == hr.shape
        return ds._dev, random.getstate()

    D = pkg.data.Degradation
    dev, state = run(D(blur_prob=1.0, noise_sigma=(1.0, 5.0)))
    assert dev.calls == ["resize_f32", "upload_f64", "blur", "resize_u8", "noise", "bicubic_of_lr"]
    random.seed(3)
    D(blur_prob=1.0, noise_sigma=(1.0, 5.0)).draw(2)
    assert random.getstate() == state

    deg = D(blur_prob=1.0, noise_sigma=(1.0, 5.0), jpeg_quality=(30, 95))
    dev, state = run(deg)
    assert dev.calls == ["resize_f32", "upload_f64", "blur", "resize_u8", "noise_bytes", "jpeg", "bicubic_of_lr"]
    random.seed(3)
    w, sigma, _ = deg.draw(2)
    q = deg.draw_jpeg(2)
    assert random.getstate() == state
    assert np.array_equal(dev.uploaded, np.concatenate([w.reshape(-1), sigma, q])) and dev.calls.count("upload_f64") == 1
    assert np.array_equal(dev.jpeg_args[0], q) and dev.jpeg_args[1:] == (1, True) and (q >= 30).all() and (q <= 95).all()

    dev, _ = run(D(blur_prob=1.0, noise_sigma=(1.0, 5.0), jpeg_quality=(30, 95), jpeg_subsampling='4:4:4'), is_gray=True)
    assert dev.jpeg_args[1:] == (0, False)          # the loader's is_gray batches are Y, Cb, Cr planes
    # JPEG alone: no blur drawn, no noise asked for -- the 8-bit shrink, then JPEG
    dev, _ = run(D(blur_prob=0.0, noise_sigma=(0.0, 0.0), jpeg_quality=(50, 50)))
    assert dev.calls == ["resize_f32", "upload_f64", "resize_u8", "jpeg", "bicubic_of_lr"]
    # on, but no patch of the batch compressed: the launches of the stages before it, and the coins are still tossed
    dev, state = run(D(blur_prob=0.0, noise_sigma=(0.0, 0.0), jpeg_quality=(50, 50), jpeg_prob=0.0))
    assert dev.calls == ["resize_f32", "resize_f32", "bicubic_of_lr"]
    random.seed(3)
    for _ in range(4):
        random.random()
    assert random.getstate() == state
    dev, _ = run(D(blur_prob=1.0, noise_sigma=(1.0, 5.0), jpeg_quality=(50, 50), jpeg_prob=0.0))
    assert dev.calls == ["resize_f32", "upload_f64", "blur", "resize_u8", "noise", "bicubic_of_lr"]


# -- command line ------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    import main as cli
    base = ["--model_name", "EDSR", "--save_dir", str(tmp_path / "out")]
    a = cli.parse_args(base)
    assert a.jpeg_quality is None and a.jpeg_prob == 1.0 and a.jpeg_subsampling == "420" and a.jpeg_test is None
    a = cli.parse_args(base + ["--degrade", "--jpeg_quality", "30,95", "--jpeg_prob", "0.8", "--jpeg_subsampling", "444",
                               "--jpeg_test", "40", "--degrade_test", "1.2,2.0,30,5"])
    assert a.degrade and a.jpeg_quality == (30, 95) and a.jpeg_prob == 0.8 and a.jpeg_subsampling == "444" \
        and a.jpeg_test == 40 and a.degrade_test == (1.2, 2.0, 30.0, 5.0)
    assert cli.parse_args(base + ["--jpeg_test", "1"]).jpeg_test == 1                      # needs no --degrade_test
    assert cli.parse_args(base + ["--degrade", "--jpeg_quality", "100,100"]).jpeg_quality == (100, 100)
    for bad in (["--jpeg_quality", "30,95"],                                                # without --degrade
                ["--degrade", "--jpeg_quality", "0,50"], ["--degrade", "--jpeg_quality", "50,101"],
                ["--degrade", "--jpeg_quality", "60,40"], ["--degrade", "--jpeg_quality", "50"],
                ["--degrade", "--jpeg_quality", "30,95,99"], ["--degrade", "--jpeg_quality", "30.5,95"],
                ["--degrade", "--jpeg_quality", "a,b"], ["--jpeg_prob", "1.5"], ["--jpeg_prob", "-0.1"], ["--jpeg_prob", "x"],
                ["--jpeg_subsampling", "422"], ["--jpeg_subsampling", "4:2:0"],
                ["--jpeg_test", "0"], ["--jpeg_test", "101"], ["--jpeg_test", "40.5"], ["--jpeg_test", "30,95"],
                ["--degrade", "--jpeg_quality", "30,95", "--synthetic"], ["--jpeg_test", "40", "--synthetic"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert "--jpeg_test" in capsys.readouterr().err


def test_trainer_refuses_jpeg_with_synthetic_or_without_degrade(pkg):
    from types import SimpleNamespace
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    for kw in (dict(jpeg_quality=(30, 95), synthetic=True), dict(jpeg_test=40, synthetic=True)):
        flag = "jpeg_quality" if "jpeg_quality" in kw else "jpeg_test"
        with pytest.raises(ValueError, match=flag):
            TRAINERS["EDSR"](SimpleNamespace(model_name="EDSR", **kw))
    with pytest.raises(ValueError, match="jpeg_quality"):
        TRAINERS["EDSR"](SimpleNamespace(model_name="EDSR", synthetic=False, degrade=False, jpeg_quality=(30, 95)))


def test_end_to_end_mirror_uses_every_path(tmp_path):
    """The loader mirror the GPU test compares against compresses some patches and leaves some alone."""
    folder = R.make_folder(str(tmp_path / "train"))
    q = [v for b in J.replay_batches(folder, 2) for v in b["quality"]]
    assert any(v == 0 for v in q) and any(v != 0 for v in q)
