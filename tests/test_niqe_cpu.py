"""NIQE without a GPU: srk_niqe_features_host (the kernels' definition in plain C++ double: same luma, window, shrink, sums
and fit, csrc/niqe_common.h) against the numpy / scipy restatement of tests/niqe_ref.py on the whole case table, the
host-made tables, the finish, the parameter file, the fit rule, every refusal and the command line.  The device kernels
are held to the same table at the same bars in tests/test_niqe_gpu.py.

Two of the table's cases have a grid of 2 x 1 blocks, so "at least 3 NaN-free rows" cannot hold for them; they are held to
"both rows NaN-free" instead, and every case with more blocks to the 3."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__
import niqe_ref as R


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def as_float(u8):
    return (u8.astype(np.float32) / np.float32(255.0)).copy()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_restatement_keeps_the_cases_conditions(name):
    """Conditions on the reference alone: its NaN rows are exactly the blocks the case made constant, and enough rows
    stay for the covariance."""
    F, _ = R.case_reference(name)
    nan_rows = np.where(np.isnan(F).any(axis=1))[0].tolist()
    assert nan_rows == R.NAN_ROWS.get(name, []), (name, nan_rows)
    for r in nan_rows:
        assert np.isnan(F[r]).all(), (name, r)     # NaN at both scales, every map
    good = F.shape[0] - len(nan_rows)
    assert good >= (3 if F.shape[0] >= 3 else 2), (name, good)
    _, (c, h, w), block, shave, _ = R.CASES[name]
    assert F.shape[0] == ((h - 2 * shave) // block) * ((w - 2 * shave) // block)


def test_the_cases_reach_what_they_are_there_for():
    alphas = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
    F = R.case_reference("grey_block8")[0][:, alphas]
    assert (F == R.GAM[0]).any() or (F == R.GAM[-1]).any()      # rn beyond the table's ends: a clamped alpha
    F = R.case_reference("remainders_nan")[0]
    assert F.shape[0] == 12 and np.isnan(F[0]).all() and not np.isnan(F[1:]).any()
    assert R.case_reference("block96")[0].shape[0] == 2 and R.case_reference("one_block_row")[0].shape[0] == 8


def test_flat_grey_passes_both_windows_exactly(pkg):
    """The premise of the constant block (niqe_ref.CASES): luma 92 comes back exactly from scipy's 49-tap sum and from the
    separable sums, so a flat region holds exact zeros for both."""
    flat = np.full((3, 16, 32), R.FLAT_GREY, np.uint8)
    assert (R.luma(flat) == 92).all()
    n, sigma = R.mscn(R.luma(flat))
    assert (n == 0).all() and (sigma == 0).all()
    F, sharp = pkg.ops.niqe_features_host(flat, 0, 16, sharpness=True)
    assert np.isnan(F).all() and (sharp == 0).all()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_host_twin_matches_the_restatement(pkg, name):
    _, _, block, shave, _ = R.CASES[name]
    F, s = R.case_reference(name)
    G, gs = pkg.ops.niqe_features_host(R.case_picture(name).copy(), shave, block, sharpness=True)
    R.assert_features(G, F, "host " + name)
    R.assert_features(gs, s, "host " + name + " sharpness")
    assert (pkg.ops.niqe_features_host(R.case_picture(name).copy(), shave, block) == G)[~np.isnan(G)].all()


def test_host_twin_reads_every_layout_to_the_same_bits(pkg):
    u8 = R.case_picture("remainders_nan").copy()
    f = as_float(u8)
    big = np.full((3, 57, 83), 0.5, np.float32)
    big[:, 4:54, 9:79] = f
    outs = [pkg.ops.niqe_features_host(a, 0, 16) for a in
            (f, np.ascontiguousarray(f.transpose(1, 2, 0)).transpose(2, 0, 1), big[:, 4:54, 9:79], u8)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0], equal_nan=True)
    R.assert_features(outs[0], R.case_reference("remainders_nan")[0], "host float picture")


def test_tables_match_scipy(pkg):
    from scipy.special import gamma
    t = pkg.ops.niqe_tables_host()
    assert t.shape == (3, 9801) and len(R.GAM) == 9801
    want = (R.R_GAM, np.sqrt(gamma(1 / R.GAM) / gamma(3 / R.GAM)), gamma(2 / R.GAM) / gamma(1 / R.GAM))
    for got, ref in zip(t, want):
        assert np.abs(got / ref - 1).max() <= 1e-13
    assert (np.diff(t[0]) > 0).all() and (np.diff(R.R_GAM) > 0).all()      # what the bisection stands on


def test_shrink_weights_are_the_cubic_at_half_scale():
    w = R.shrink_weights_from_formula()
    assert np.array_equal(w, R.SHRINK) and w.sum() == 1.0
    assert np.array_equal(R.SHRINK * 256, [-3, -9, 29, 111, 111, 29, -9, -3])
    ramp = np.add.outer(np.arange(32.0), 2 * np.arange(48.0))
    want = np.add.outer(2 * np.arange(16.0) + 0.5, 2 * (2 * np.arange(24.0) + 0.5))
    assert np.array_equal(R.shrink(ramp)[2:-2, 2:-2], want[2:-2, 2:-2])    # a cubic reproduces a ramp away from the edges


def test_finish_and_the_score(pkg):
    mu_p, cov_p, rows = R.fitted_params()
    assert rows >= 37 and np.linalg.cond(cov_p) <= R.COND_MAX
    for name in ("remainders_nan", "grey_block8"):
        _, _, block, shave, _ = R.CASES[name]
        want = R.finish(R.case_reference(name)[0], mu_p, cov_p)
        got = pkg.ops.niqe_finish(pkg.ops.niqe_features_host(R.case_picture(name).copy(), shave, block), mu_p, cov_p)
        print("%s: niqe %.9f (restatement %.9f)" % (name, got, want))
        assert abs(got - want) <= R.SCORE_RTOL * want
        assert pkg.ops.niqe_finish(R.case_reference(name)[0], mu_p.reshape(1, 36), cov_p) == want
    F = np.array(R.case_reference("2x2_exact")[0])
    F[1:, 3] = np.nan
    with pytest.raises(ValueError, match="1 of 4 blocks"):
        pkg.ops.niqe_finish(F, mu_p, cov_p)
    with pytest.raises(ValueError, match=r"are not \[blocks, 36\]"):
        pkg.ops.niqe_finish(F[:, :35], mu_p, cov_p)


def test_parameter_file_round_trip_and_key_names(pkg, tmp_path):
    mu_p, cov_p, _ = R.fitted_params()
    path = tmp_path / "p.npz"
    pkg.utils.save_niqe_params(path, mu_p, cov_p)
    assert np.load(path)["mu_pris_param"].shape == (1, 36)
    mu, cov = pkg.utils.load_niqe_params(path)
    assert mu.shape == (36,) and np.array_equal(mu, mu_p) and np.array_equal(cov, cov_p)
    np.savez(tmp_path / "flat.npz", mu_pris_param=mu_p, cov_pris_param=cov_p, gaussian_window=np.ones((7, 7)))
    mu, cov = pkg.utils.load_niqe_params(tmp_path / "flat.npz")
    assert np.array_equal(mu, mu_p) and np.array_equal(cov, cov_p)
    np.savez(tmp_path / "nomu.npz", cov_pris_param=cov_p)
    with pytest.raises(KeyError, match="mu_pris_param"):
        pkg.utils.load_niqe_params(tmp_path / "nomu.npz")
    np.savez(tmp_path / "nocov.npz", mu_pris_param=mu_p, cov=cov_p)
    with pytest.raises(KeyError, match="cov_pris_param"):
        pkg.utils.load_niqe_params(tmp_path / "nocov.npz")
    np.savez(tmp_path / "shape.npz", mu_pris_param=mu_p[:35], cov_pris_param=cov_p)
    with pytest.raises(ValueError, match="are not"):
        pkg.utils.load_niqe_params(tmp_path / "shape.npz")
    metric = pkg.utils.NIQE(path, shave=2, block=16)
    assert np.array_equal(metric.params[0], mu_p) and (metric.shave, metric.block) == (2, 16)


def test_fit_rule_with_the_host_twin(pkg):
    pictures = [R.picture(100 + i, 3, 64, 80) for i in range(8)]
    mu_p, cov_p, rows = R.fitted_params()
    mu, cov, n = pkg.utils.fit_niqe_params(pictures, block=16, host=True)
    assert n == rows
    assert np.abs(mu - mu_p).max() <= 1e-9 * max(1.0, np.abs(mu_p).max())
    assert np.abs(cov - cov_p).max() <= 1e-9 * max(1.0, np.abs(cov_p).max())
    # the rule itself, on made-up rows: sharpness above 0.75 of the picture's maximum, no NaN
    f = np.arange(4 * 36, dtype=np.float64).reshape(4, 36)
    f[3, 5] = np.nan
    with pytest.raises(ValueError, match="2 blocks pass"):
        pkg.utils.pool_niqe_rows([(f, np.array([4.0, 3.0, 3.04, 4.0]))])   # 3.0 is not above 0.75 * 4; row 3 has a NaN
    with pytest.raises(ValueError, match="at least 37"):
        pkg.utils.fit_niqe_params(pictures[:1], block=16, host=True)
    many = np.random.RandomState(0).rand(60, 36)
    s = np.ones(60)
    s[:10] = 0.5
    mu, cov, n = pkg.utils.pool_niqe_rows([(many, s)])
    assert n == 50 and np.array_equal(mu, many[10:].mean(0)) and np.array_equal(cov, np.cov(many[10:], rowvar=False))


def test_table_search_is_argmin(pkg):
    """The bisection and neighbour comparison against np.argmin through the fit: blocks of 4 x 4 values scatter rn over
    and beyond the table."""
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (1, 48, 64)).astype(np.uint8)
    F = pkg.ops.niqe_features_host(img, 0, 8)
    W = R.features(img, 0, 8)
    R.assert_features(F, W, "random bytes, block 8")
    alphas = W[:, [18, 20, 24, 28, 32]]
    assert len(np.unique(alphas[~np.isnan(alphas)])) > 50


def test_every_refusal_names_its_number(pkg, lib):
    tables = pkg.ops.niqe_tables_host()
    img = np.zeros((3, 64, 64), np.uint8)
    feats = np.zeros((16, 36))

    def call(fn, img=img, c=3, h=64, w=64, shave=0, block=16, tables=tables, feats=feats, extra=()):
        p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        return fn(p(img), 1, None, c, h, w, shave, block, p(tables), p(feats), None, *extra)

    for fn, extra in ((lib.srk_niqe_features_host, ()), (lib.srk_niqe_features, (ctypes.c_void_p(64), None))):
        for kw, match in ((dict(block=15), b"even and in 8 .. 96 (got 15)"), (dict(block=98), b"(got 98)"),
                          (dict(block=6), b"(got 6)"), (dict(c=2), b"1 or 3 channels (got 2)"),
                          (dict(h=40, w=31, block=24), b"40 x 31 with 0 pixels shaved from each side holds 1 x 1 blocks of 24 x 24"),
                          (dict(shave=20, block=24), b"64 x 64 with 20 pixels shaved from each side holds 1 x 1 blocks"),
                          (dict(shave=-1), b"negative shave (-1)"), (dict(img=None), b"null pointer"),
                          (dict(tables=None), b"null pointer"), (dict(feats=None), b"null pointer")):
            assert call(fn, extra=extra, **kw) == -1, kw
            assert match in lib.srk_last_error_string(), (kw, lib.srk_last_error_string())
    assert call(lib.srk_niqe_features, extra=(None, None)) == -1 and b"null workspace" in lib.srk_last_error_string()
    assert lib.srk_niqe_tables_host(None) == -1 and b"null pointer" in lib.srk_last_error_string()
    assert lib.srk_niqe_workspace_bytes(197, 99, 96) == 2 * 48 * 48 * 8
    assert lib.srk_niqe_workspace_bytes(64, 64, 15) == 0 and lib.srk_niqe_workspace_bytes(0, 64, 16) == 0
    import torch
    for bad, match in ((dict(block=15), "got 15"), (dict(shave=-2), "negative shave"), (dict(block=64), "fewer than 2")):
        with pytest.raises(ValueError, match=match):
            pkg.ops.niqe_features_host(img, **bad)
    with pytest.raises(ValueError, match="C in"):
        pkg.ops.niqe_features_host(np.zeros((2, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="float32 or a uint8"):
        pkg.ops.niqe_features_host(np.zeros((3, 64, 64), np.float64))
    with pytest.raises(RuntimeError, match="must be on the device"):
        pkg.ops.niqe_features(torch.zeros(3, 64, 64), block=16)


def test_cli_carries_the_niqe_flags(tmp_path, capsys):
    import main as cli
    base = ["--save_dir", str(tmp_path)]
    plain = cli.parse_args(base)
    assert plain.niqe_params is None and plain.niqe_fit is None
    params = tmp_path / "p.npz"
    mu_p, cov_p, _ = R.fitted_params()
    np.savez(params, mu_pris_param=mu_p, cov_pris_param=cov_p)
    a = cli.parse_args(base + ["--test_only", "--niqe_params", str(params), "--eval_shave", "4"])
    assert a.niqe_params == str(params) and a.niqe_fit is None and a.test_only
    same = {k: v for k, v in vars(a).items() if k not in ("niqe_params", "test_only", "eval_shave")}
    assert same == {k: v for k, v in vars(plain).items() if k not in ("niqe_params", "test_only", "eval_shave")}
    pics = tmp_path / "pics"
    pics.mkdir()
    fit = cli.parse_args(base + ["--niqe_fit", str(pics), "--niqe_params", str(tmp_path / "new.npz")])
    assert fit.niqe_fit == str(pics)
    for argv, match in ((["--niqe_params", str(tmp_path / "missing.npz")], "missing.npz: no such file"),
                        (["--niqe_fit", str(pics)], "needs --niqe_params OUT"),
                        (["--niqe_fit", str(pics), "--niqe_params", str(params)], "does not overwrite"),
                        (["--niqe_fit", str(tmp_path / "nodir"), "--niqe_params", str(tmp_path / "n.npz")], "no such directory"),
                        (["--niqe_fit", str(pics), "--niqe_params", str(tmp_path / "n.npz"), "--test_only"],
                         "does not go with --test_only"),
                        (["--niqe_fit", str(pics), "--niqe_params", str(tmp_path / "n.npz"), "--test_single", "x.png"],
                         "does not go with --test_single")):
        with pytest.raises(SystemExit):
            cli.parse_args(base + argv)
        assert match in capsys.readouterr().err, argv


def test_header_integration_and_build_name_the_new_unit(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for sym in ("srk_niqe_tables_host", "srk_niqe_workspace_bytes", "srk_niqe_features", "srk_niqe_features_host"):
        assert sym in pkg._lib.header_symbols() and sym in pkg._lib._PROTOTYPES
        assert sym in open(os.path.join(root, "INTEGRATION.md")).read(), sym
    assert "niqe.hip" in pkg._build.SOURCES and "niqe_common.h" in pkg._build.HEADERS
