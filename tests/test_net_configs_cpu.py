"""The configuration matrix of tests/net_configs_ref.py on the CPU: its inputs are well conditioned, and its layer table is
what its derivation gives.

Conditioning: tests/test_net_configs_gpu.py holds the package's fp32 kernels to bars against the fp64 oracle.  A bar only
tests the kernels when plain fp32 arithmetic clears it with room: here each configuration's oracle runs in fp32 and in fp64
on the same inputs, and fp32 must land within ONE QUARTER of every bar -- the GPU's different summation order then has the
same room again, twice over.  A configuration that misses the quarter gets another input seed, never another bar.  Run with
-s, the test prints the worst share of each configuration: that print is the record."""
import pytest
import torch

import net_configs_ref as N

QUARTER = 0.25


def _check(name, rows):
    what, bar, used = N.worst(rows)
    print("%-22s fp32 vs fp64 oracle: %3d checks, worst %.4f of its bar (%s, %s)" % (name, len(rows), used, what, bar))
    bad = [r for r in rows if not r[2] <= QUARTER]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", N.NET_CONFIGS)
def test_fp32_oracle_within_a_quarter_of_every_bar(name):
    """Outputs (element-wise 1e-3 and max-norm 1e-4), dx, every parameter gradient (element-wise 1e-3; the zero-gradient
    rule where it applies), BatchNorm buffers and the eval-mode forward."""
    _check(name, N.compare(name, N.run_oracle_fp32(name), N.run_oracle(name)))


@pytest.mark.parametrize("name", N.DISC_CONFIGS)
def test_fp32_discriminator_forward_within_a_quarter(name):
    """The discriminator is held on its train-mode output, its running statistics and its eval-mode output only (its
    gradients: tests/test_net_configs_gpu.py says why), so these are what must be well conditioned."""
    _check(name, N.compare(name, N.run_oracle_fp32(name, backward=False), N.run_oracle(name, backward=False)))


def test_matrix_is_complete():
    names = set(N.CONFIGS)
    for c in (1, 3):
        for net in ("srcnn", "vdsr", "edsr", "lapsrn", "srgan_g"):
            assert "%s_c%d" % (net, c) in names
        assert {"espcn_c%d_x%d" % (c, r) for r in (2, 3, 4, 8)} <= names
        assert {"fsrcnn_c%d_x%d" % (c, r) for r in (2, 3, 4)} <= names
        assert {"rcan_c%d_x%d" % (c, r) for r in (2, 4, 8)} <= names
        assert {"srgan_d_c%d_crop%d" % (c, s) for s in (16, 32, 48, 96)} <= names
    assert len(names) == 10 + 8 + 6 + 6 + 8
    # the (3 channels, scale 4) points are test_nets_gpu.CASES, shape and gain included
    import test_nets_gpu as T
    same = {"srcnn": "srcnn_c3", "espcn": "espcn_c3_x4", "fsrcnn": "fsrcnn_c3_x4", "vdsr": "vdsr_c3", "edsr": "edsr_c3",
            "lapsrn": "lapsrn_c3", "srgan_g": "srgan_g_c3"}
    for old, new in same.items():
        cls, args, ishape, gain = T.CASES[old]
        cfg = N.CONFIGS[new]
        assert (cfg.product, cfg.args, cfg.ishape, cfg.gain) == (cls, args, ishape, gain), new
        assert N.oracle_class(cfg) is T.ORACLES[old]


def test_layer_table_matches_its_derivation():
    """LAYER_ROWS is the walk of every configuration's oracle minus what CONV_KATS and test_ops_gpu.py's parametrisations
    already run; it fails when a configuration, an oracle or one of those tables has moved."""
    assert N.LAYER_ROWS == N.derive_layer_rows()
    assert len({r[:9] for r in N.LAYER_ROWS}) == len(N.LAYER_ROWS)
    assert all(r[9] in N.CONFIGS for r in N.LAYER_ROWS)
    keys = {r[:9] for r in N.LAYER_ROWS}
    # what the walk must have found, by kernel-dispatch class
    for k, p in ((3, 1), (5, 0), (9, 0), (9, 4)):
        assert any(r[0] == "conv" and r[1] == 1 and r[3] == k and r[5] == p for r in keys), ("Cin = 1", k, p)
    for cin, k in ((64, 3), (32, 5), (64, 9)):
        assert any(r[0] == "conv" and r[1] == cin and r[2] == 1 and r[3] == k for r in keys), ("Cout = 1", cin, k)
    tails = {(r[2], r[8]) for r in keys if r[0] == "conv" and r[1] == 32 and r[8]}
    assert tails == {(4, 2), (9, 3), (16, 4), (64, 8), (12, 2), (27, 3), (192, 8)}     # x4 RGB: CONV_KATS / test_ops_gpu.py
    assert {(r[2], r[4]) for r in keys if r[0] == "deconv" and r[3] == 9} == {(1, 2), (1, 3), (1, 4), (3, 2), (3, 3)}
    assert ("deconv", 1, 1, 4, 2, 1, 0, None, 0) in keys
    assert {r[1] for r in keys if r[0] == "linear" and r[2] == 1024} == {512, 2048, 4608, 18432}
    assert ("linear", 1024, 1, 0, 0, 0, 0, "sigmoid", 0) in keys


def test_layer_references_agree_with_an_independent_composition():
    """row_reference (activation, then shuffle) equals the blocks' order (shuffle, then activation) for the fused tails."""
    for i, row in enumerate(N.LAYER_ROWS):
        if row[0] == "linear" or not row[8] or row[7] is None:
            continue
        x, w, b, slope = N.row_inputs(i)
        z = torch.nn.functional.pixel_shuffle(N.row_linear_part(i, x.double(), w.double(), b.double()), row[8])
        assert torch.equal(N.apply_act(z, row[7], slope), N.row_reference(i))
