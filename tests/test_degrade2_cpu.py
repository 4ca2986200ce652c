"""Real-ESRGAN's second-order degradation without a GPU: the host-made tables against degrade2_ref.py and
scipy, the host twins of the noise and unsharp-mask kernels byte for byte against the numpy restatement, the guard that
lets the byte-equal tests (here and on the GPU) demand zero mismatches -- no value of the case tables rounds within 1e-7 of
a boundary -- the draws from Python's `random`, the refusals and the exported symbols."""
import ctypes
import json
import math
import random

import numpy as np
import pytest

import __graft_entry__
import degrade_ref as R1
import degrade2_ref as R

INVALID = -1   # SRK_ERR_INVALID (= SRK_ERR_BAD_ARG, include/srk.h)
NEW_SYMBOLS = ["srk_blur_table_host", "srk_poisson_cdf_host", "srk_noise2_u8", "srk_noise2_u8_host", "srk_usm_table_host",
               "srk_usm_u8_workspace_bytes", "srk_usm_u8", "srk_usm_u8_host"]


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def cdf_lib(pkg):
    return pkg.ops.poisson_cdf()


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_noise2(lib, x, mode, gray, amount, cdf, seed, stage, color):
    x = np.ascontiguousarray(x)
    y = np.full_like(x, 77)
    B, C, H, W = x.shape
    rc = lib.srk_noise2_u8_host(vp(x), vp(y), vp(mode), vp(gray), vp(amount), vp(cdf), seed, stage, B, C, H, W, int(color))
    assert rc == 0, lib.srk_last_error_string()
    return y


def host_usm(lib, x, g, weight, threshold):
    x = np.ascontiguousarray(x)
    y = np.full_like(x, 77)
    B, C, H, W = x.shape
    rc = lib.srk_usm_u8_host(vp(x), vp(y), vp(g), len(g), weight, threshold, B, C, H, W)
    assert rc == 0, lib.srk_last_error_string()
    return y


# -- tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.TABLE_KS)
@pytest.mark.parametrize("case", R.TABLE_CASES, ids=lambda c: "%s-%g-%g" % (c[0], c[1], c[5]))
def test_blur_table_matches_mirror(pkg, K, case):
    """The library's table against the mirror's (math.fsum normalisation; sinc through scipy.special.j1).  The two differ by
    what libm and Python / scipy round, so the bar is the mirror's own rounding: its largest difference from a second
    evaluation in numpy.longdouble, times 4 (floored at one ulp of the table's largest entry, the least any two fp64
    evaluations can be told apart by).  Measured over these 24 cases: mirror against longdouble at most 3.33e-16 (a
    sinc table's centre tap, which takes up the residual of the normalisation), library against mirror at most 1.11e-16."""
    kind = case[0]
    got = pkg.ops.blur_table(kind, K, *case[1:])
    want = R.blur_table(kind, K, *case[1:])
    second = R.blur_table_longdouble(kind, K, *case[1:])
    own = float(np.abs(want - second).max())
    bar = max(4.0 * own, float(np.spacing(np.abs(want).max())))
    err = float(np.abs(got - want).max())
    print("blur_table %s K %d: library - mirror %.3g, mirror - longdouble %.3g" % (kind, K, err, own))
    assert got.shape == (K, K) and err <= bar
    assert abs(math.fsum(got.ravel()) - 1.0) <= 2.2e-16
    if kind == "sinc":
        assert got.min() < 0.0 and (got < 0.0).sum() >= 4


def test_blur_table_refusals(lib):
    w = (ctypes.c_double * 441)()
    assert lib.srk_blur_table_host(0, 7, 1.0, 1.0, 0.0, 1.0, 1.0, None) == INVALID
    for K in (5, 8, 23):
        assert lib.srk_blur_table_host(0, K, 1.0, 1.0, 0.0, 1.0, 1.0, w) == INVALID
    assert lib.srk_blur_table_host(4, 7, 1.0, 1.0, 0.0, 1.0, 1.0, w) == INVALID
    assert lib.srk_blur_table_host(0, 7, 0.0, 1.0, 0.0, 1.0, 1.0, w) == INVALID
    assert lib.srk_blur_table_host(1, 7, 1.0, 1.0, 0.0, 0.0, 1.0, w) == INVALID
    assert lib.srk_blur_table_host(3, 7, 1.0, 1.0, 0.0, 1.0, 0.0, w) == INVALID


def test_poisson_table(cdf_lib):
    """Rows non-decreasing and ending at exactly 1.0, row 0 all ones, the mass beyond column KT - 2 below 2^-33, and the
    whole table against scipy.stats.poisson.cdf: measured 2.55e-15 at most (scipy sums through the incomplete gamma
    function; a running product over 447 terms carries about that much)."""
    from scipy.stats import poisson
    assert cdf_lib.shape == (256, R.KT)
    assert (np.diff(cdf_lib, axis=1) >= 0.0).all() and (cdf_lib[:, -1] == 1.0).all() and (cdf_lib[0] == 1.0).all()
    assert (cdf_lib[:, R.KT - 2] >= 1.0 - 2.0 ** -33).all()
    lam = np.arange(256, dtype=np.float64)[:, None] * R.PEAK / 255.0
    err = float(np.abs(cdf_lib - poisson.cdf(np.arange(R.KT)[None, :], lam)).max())
    print("poisson table against scipy: %.3g" % err)
    assert err <= 1e-13      # 447 products and sums of fp64 roundings, 2^-53 each, with room: 447 * 2 * 1.1e-16
    assert (cdf_lib == R.cdf()).all()     # the mirror's pure-Python restatement makes the same bits (one libm exp)


# -- the noise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NOISE2_CPU)
def test_noise2_host_is_byte_equal(lib, cdf_lib, name):
    x, mode, gray, amount, seed, stage, color = R.noise2_case(name)
    got = host_noise2(lib, x, mode, gray, amount, cdf_lib, seed, stage, color)
    want = R.noise2(x, mode, gray, amount, cdf_lib, seed, stage, color)
    assert int((got != want).sum()) == 0
    off = mode == 0
    assert (got[off] == x[off]).all()


def test_noise2_colour_gauss_is_noise_u8_bytes(lib, cdf_lib):
    """Stage 0, colour, Gaussian: the existing srk_noise_u8_bytes mirror's bytes (degrade_ref.noise x 255)."""
    for name in [c[0] for c in R1.NOISE_CASES]:
        x, sigma, seed = R1.noise_case(name)
        if x.shape[1] not in (1, 3):
            continue
        x4 = x.reshape(x.shape[0], x.shape[1], x.shape[2], -1)
        B = x4.shape[0]
        got = host_noise2(lib, x4, np.ones(B), np.zeros(B), sigma, cdf_lib, seed, 0, True)
        want = np.round(R1.noise(x, sigma, seed) * 255.0).astype(np.uint8)
        assert int((got.reshape(x.shape) != want).sum()) == 0


def test_noise2_refusals(lib, cdf_lib):
    x = np.zeros((1, 3, 4, 4), np.uint8)
    one = np.ones(1)
    args = lambda **k: [k.get('x', vp(x)), vp(x), vp(one), vp(one), vp(one), k.get('cdf', vp(cdf_lib)), 1, k.get('stage', 1),
                        1, k.get('C', 3), k.get('H', 4), 4, 1]
    assert lib.srk_noise2_u8_host(*args()) == 0
    for bad in (dict(x=None), dict(cdf=None), dict(C=2), dict(H=0), dict(stage=3)):
        assert lib.srk_noise2_u8_host(*args(**bad)) == INVALID
        assert lib.srk_noise2_u8(*(args(**bad) + [None])) == INVALID      # refused before anything is launched


# -- the unsharp mask ---------------------------------------------------------------------------------------------------
def test_usm_table(pkg):
    g = pkg.ops.usm_table()
    assert len(g) == 51 and abs(math.fsum(g) - 1.0) <= 2.2e-16
    assert float(np.abs(g - R.usm_table()).max()) <= float(np.spacing(g.max()))
    assert float(np.abs(pkg.ops.usm_table(5, 1.1) - R.usm_table(5, 1.1)).max()) <= 1.2e-16


@pytest.mark.parametrize("name", R.USM_CPU)
def test_usm_host_is_byte_equal(lib, pkg, name):
    x, g, weight, threshold = R.usm_case(name)
    got = host_usm(lib, x, pkg.ops.usm_table(len(g)), weight, threshold)
    assert int((got != R.usm(x, g, weight, threshold)).sum()) == 0


def test_usm_identities(lib, pkg):
    g = pkg.ops.usm_table()
    flat = np.full((1, 3, 30, 41), 137, np.uint8)
    assert (host_usm(lib, flat, g, 0.5, 10.0) == flat).all()            # a constant plane returns itself
    x = R.usm_case("radius_25")[0]
    assert (host_usm(lib, x, g, 0.5, 255.0) == x).all()                 # nothing exceeds the threshold: the input


def test_usm_refusals(lib, pkg):
    g = pkg.ops.usm_table()
    x = np.zeros((1, 3, 26, 26), np.uint8)
    ok = lambda **k: lib.srk_usm_u8_host(k.get('x', vp(x)), vp(x), k.get('g', vp(g)), k.get('K', 51), 0.5, 10.0, 1,
                                         k.get('C', 3), k.get('H', 26), 26)
    assert ok() == 0
    for bad in (dict(x=None), dict(g=None), dict(K=50), dict(K=53), dict(C=2), dict(H=25)):
        assert ok(**bad) == INVALID
    dev = lambda **k: lib.srk_usm_u8(vp(x), vp(x), vp(g), k.get('K', 51), 0.5, 10.0, 1, k.get('C', 3), k.get('H', 26), 26,
                                     vp(x), 1 << 30, None)
    for bad in (dict(K=50), dict(K=53), dict(C=2), dict(H=25)):
        assert dev(**bad) == INVALID
    assert lib.srk_usm_u8_workspace_bytes(2, 3, 27, 40) >= 2 * 3 * 27 * 40 * 9


# -- boundary margins ---------------------------------------------------------------------------------------------------
def test_case_tables_keep_their_margins():
    """a byte-equal test must not depend on one side's last rounding.  Every case the byte-equal tests use,
    here and on the GPU, keeps its pre-rounding values 1e-7 away from a rounding boundary and |R| 1e-7 from the threshold."""
    for c in R.NOISE2_CASES:
        x, mode, gray, amount, seed, stage, color = R.noise2_case(c[0])
        assert R.noise2_margin(R.noise2_pre(x, mode, gray, amount, R.cdf(), seed, stage, color), mode) > R.GUARD, c[0]
    for c in R.USM_CASES:
        x, g, weight, threshold = R.usm_case(c[0])
        pre, resid = R.usm_parts(x, g, weight, threshold)
        assert R.margin(pre) > R.GUARD and float(np.abs(resid).min()) > R.GUARD, c[0]
    for iseed, shape in R.BLUR2_SHAPES:
        for t in R.BLUR2_TABLES:
            w = np.stack([R.blur_table(*t)] * shape[0])
            assert R.margin(R1.blur_pre(R1.image(iseed, shape), w)) > R.GUARD, (shape, t)


def test_chain_cases_keep_their_margins(tmp_path):
    """The same guard for the whole chain on the batches and the test items the GPU tests replay, and the set of things
    those batches exercise."""
    from PIL import Image
    folder = R.make_folder(str(tmp_path / "train"))
    drawn = []
    for gray in (False, True):
        for usm_on in (False, True):
            for seed in R.E2E_SEEDS:
                ref = R.replay_batch(folder, seed, is_gray=gray, usm_on=usm_on)
                assert ref['guard'] > R.GUARD, (gray, usm_on, seed, ref['guard'])
                drawn.append(ref['p'])
    assert R.coverage(drawn) >= R.WANTED
    import os
    for i, fn in enumerate(sorted(os.listdir(folder))):
        hwc = np.asarray(Image.open(os.path.join(folder, fn)).convert('RGB'), dtype=np.uint8)
        assert R.test_item(hwc, R.E2E['scale_factor'], R.TEST_SEED, i)[1] > R.GUARD, fn


# -- BOX ------------------------------------------------------------------------------------------------------------------
def test_box_is_a_filter_code(pkg):
    from PIL import Image
    assert pkg.ops.INTERP_BOX == int(Image.BOX) == R.BOX and pkg.data.BOX == R.BOX and pkg.data.BILINEAR == int(Image.BILINEAR)


# -- draws --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert set(k for k in a if not k.startswith('spec')) == set(k for k in b if not k.startswith('spec'))
    for k, v in a.items():
        if k.startswith('spec'):
            continue
        if isinstance(v, dict):
            for f in v:
                assert np.array_equal(np.asarray(v[f]), np.asarray(b[k][f])), (k, f)
        elif k in ('k1', 'k2', 'k3'):
            assert v.shape == b[k].shape and float(np.abs(v - b[k]).max()) <= 1e-15, k     # (libm's j1 against scipy's)
        else:
            assert np.array_equal(np.asarray(v), np.asarray(b[k])), k


def test_draw_replays_and_matches_mirror(pkg):
    d = pkg.data.Degradation2(resize_range=(0.5, 1.5))
    random.seed(11)
    state = random.getstate()
    first = [d.draw(4) for _ in range(3)]
    after = random.getstate()
    random.setstate(state)
    again = [d.draw(4) for _ in range(3)]
    for a, b in zip(first, again):
        _same(a, b)
    random.setstate(state)
    for a in first:
        _same(a, {k: v for k, v in R.draw(4, random, resize_range=(0.5, 1.5)).items()})
    assert random.getstate() == after
    rng = random.Random(5)                       # a private generator leaves the global one alone
    d.draw(2, rng)
    assert random.getstate() == after


def test_other_loaders_consume_the_draws_they_did(pkg):
    """degrade=None or a Degradation: the datasets' draws are the recorded ones -- Degradation.draw / draw_jpeg consume what
    the restatement of the parent's classes (degrade_ref.draw, jpeg_ref.draw_jpeg) consumes, and a dataset without a
    degradation consumes nothing beyond its patch draws."""
    import jpeg_ref as J
    kw = dict(blur_prob=0.5, blur_sigma=(0.4, 3.5), noise_sigma=(1.0, 12.0))
    random.seed(3)
    R1.draw(4, kw['blur_prob'], kw['blur_sigma'], kw['noise_sigma'])
    J.draw_jpeg(4, (30, 90), 0.7)
    recorded = random.getstate()
    d = pkg.data.Degradation(jpeg_quality=(30, 90), jpeg_prob=0.7, **kw)
    random.seed(3)
    d.draw(4)
    d.draw_jpeg(4)
    assert random.getstate() == recorded
    ds = pkg.data.TrainDatasetFromFolder([], crop_size=32, scale_factor=4, degrade=None)
    from oracle import dataset_pil as O
    random.seed(4)
    ds.draw(64, 48)
    mine = random.getstate()
    assert ds.usm is False and ds.degrade is None
    random.seed(4)
    pkg.data.TrainDatasetFromFolder([], crop_size=32, scale_factor=4, degrade=d).draw(64, 48)
    assert random.getstate() == mine


# -- refusals -----------------------------------------------------------------------------------------------------------
def test_unknown_setting_is_named(pkg):
    with pytest.raises(ValueError, match="resize_rnage"):
        pkg.data.Degradation2(resize_rnage=(0.5, 1.5))
    with pytest.raises(ValueError, match="jpeg_range2"):
        pkg.data.Degradation2(jpeg_range2=(0, 50))
    with pytest.raises(ValueError, match="kernel_sizes"):
        pkg.data.Degradation2(kernel_sizes=(8,))


def test_crop_and_scale_are_checked_where_the_dataset_binds(pkg):
    d = pkg.data.Degradation2()
    pkg.data.TrainDatasetFromFolder([], crop_size=128, scale_factor=4, degrade=d)          # the defaults pass
    with pytest.raises(ValueError, match="resize_range"):
        pkg.data.TrainDatasetFromFolder([], crop_size=48, scale_factor=4, degrade=d)       # int(48 * 0.15) = 7
    with pytest.raises(ValueError, match="resize_range"):
        pkg.data.TrainDatasetFromFolder([], crop_size=40, scale_factor=4, degrade=pkg.data.Degradation2(resize_range=(0.5, 1.5)))
    with pytest.raises(ValueError, match="usm"):
        pkg.data.TrainDatasetFromFolder([], crop_size=24, scale_factor=4, usm=True)


def _main_error(capsys, argv):
    import main
    with pytest.raises(SystemExit):
        main.parse_args(argv)
    return capsys.readouterr().err


def test_command_line_refusals(capsys, tmp_path):
    base = ['--model_name', 'EDSR', '--save_dir', str(tmp_path)]
    err = _main_error(capsys, base + ['--degrade', '--degrade2'])
    assert '--degrade2' in err and '--degrade' in err
    assert '--jpeg_quality' in _main_error(capsys, base + ['--degrade2', '--jpeg_quality', '30,90'])
    assert '--degrade2' in _main_error(capsys, base + ['--degrade2', '--synthetic'])
    assert '--usm' in _main_error(capsys, base + ['--usm', '--synthetic'])
    assert '--degrade2_test' in _main_error(capsys, base + ['--degrade2_test', '3', '--synthetic'])
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"resize_range": [0.5, 1.5], "blurr_sigma": [0.2, 2.0]}))
    assert 'blurr_sigma' in _main_error(capsys, base + ['--degrade2', str(bad)])
    good = tmp_path / "good.json"
    good.write_text(json.dumps({"resize_range": [0.5, 1.5]}))
    import main
    args = main.parse_args(base + ['--degrade2', str(good), '--usm', '--degrade2_test', '9'])
    assert args.degrade2 == {"resize_range": [0.5, 1.5]} and args.usm and args.degrade2_test == 9
    args = main.parse_args(base + ['--degrade2'])
    assert args.degrade2 == {}
    args = main.parse_args(base)
    assert args.degrade2 is None and not args.usm and args.degrade2_test is None


def test_settings_keys_are_the_class_keywords(pkg):
    import main
    assert sorted(main.DEGRADE2_KEYS) == sorted(pkg.data.Degradation2.DEFAULTS)
    assert sorted(k for k in pkg.data.Degradation2.DEFAULTS if k != 'jpeg_subsampling') == sorted(R.DEFAULTS)
    for k, v in R.DEFAULTS.items():
        assert pkg.data.Degradation2.DEFAULTS[k] == v, k


def test_trainer_refuses_synthetic(pkg):
    import types
    from pytorch_super_resolution_model_collection_amd import sr_trainers
    for flag, value in (("degrade2", {}), ("usm", True), ("degrade2_test", 3)):
        args = types.SimpleNamespace(synthetic=True, **{flag: value})
        with pytest.raises(ValueError, match=flag):
            sr_trainers.check_data_flags(args)
    with pytest.raises(ValueError, match="degrade2"):
        sr_trainers.check_data_flags(types.SimpleNamespace(synthetic=False, degrade=True, degrade2={}))
    with pytest.raises(ValueError, match="jpeg_quality"):
        sr_trainers.check_data_flags(types.SimpleNamespace(synthetic=False, degrade2={}, jpeg_quality=(30, 90)))


# -- symbols ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(pkg, lib):
    declared = pkg._lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib._PROTOTYPES and getattr(lib, name) is not None
    for name in ("noise2_u8", "usm_u8", "blur_table", "poisson_cdf"):
        assert callable(getattr(pkg.ops, name))
