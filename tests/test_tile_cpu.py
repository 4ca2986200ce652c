"""tiling.py on the host: the derived dependency cones against the NaN support of the reference nets (both directions),
the plan's invariants checked exhaustively in integers, and stitching by the plan in fp64 against the one-pass oracle."""
import itertools

import pytest
import torch

from oracle import fill, ref_modules as R


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd import tiling
    return pkg, tiling


R4 = 4
# name -> (product net, oracle twin, (H, W) of the probe picture) per depth.  Widths are small: geometry does not read them.
NETS = {
    "SRCNN": [(lambda M: M.SRCNNNet(1, 8), lambda: R.SRCNN(1, 8), (40, 37))],
    "ESPCN": [(lambda M: M.ESPCNNet(1, 8, R4), lambda: R.ESPCN(1, 8, R4), (31, 29)),
              (lambda M: M.ESPCNNet(1, 8, 3), lambda: R.ESPCN(1, 8, 3), (23, 20))],
    "FSRCNN": [(lambda M: M.FSRCNNNet(1, R4, 8, 4, 4), lambda: R.FSRCNN(1, R4, 8, 4, 4), (41, 37)),
               (lambda M: M.FSRCNNNet(1, 2, 8, 4, 2), lambda: R.FSRCNN(1, 2, 8, 4, 2), (29, 31))],
    "VDSR": [(lambda M: M.VDSRNet(1, 4, 18), lambda: R.VDSR(1, 4, 18), (61, 53)),
             (lambda M: M.VDSRNet(1, 4, 3), lambda: R.VDSR(1, 4, 3), (23, 29))],
    "EDSR": [(lambda M: M.EDSRNet(3, 4, 16), lambda: R.EDSR(3, 4, 16), (89, 83)),
             (lambda M: M.EDSRNet(3, 4, 2), lambda: R.EDSR(3, 4, 2), (29, 23))],
    "LapSRN": [(lambda M: M.LapSRNNet(1, 4, 10), lambda: R.LapSRN(1, 4, 10), (47, 43)),
               (lambda M: M.LapSRNNet(1, 4, 2), lambda: R.LapSRN(1, 4, 2), (23, 19))],
    "SRGAN": [(lambda M: M.SRGANGenerator(3, 4, 16), lambda: R.Generator(3, 4, 16), (97, 89)),
              (lambda M: M.SRGANGenerator(3, 4, 1), lambda: R.Generator(3, 4, 1), (31, 29))],
}
CASES = [(name, i) for name in sorted(NETS) for i in range(len(NETS[name]))]


def _geometry(name, i):
    pkg, tiling = _pkg()
    return tiling.net_geometry(NETS[name][i][0](pkg.models).eval())


def _last(out):
    return out[-1] if isinstance(out, (tuple, list)) else out


def _positions(h, w):
    """interior, near each edge, a corner"""
    return [(h // 2, w // 2), (1, w // 2), (h - 2, w // 3), (h // 3, 0), (h // 2, w - 1), (0, 0), (h - 1, w - 1)]


@pytest.mark.parametrize("name,i", CASES, ids=["%s-%d" % c for c in CASES])
def test_cone_equals_nan_support(name, i):
    """One NaN pixel in a finite picture: NaN passes every conv tap, ReLU, PReLU, eval BatchNorm and add, so the NaN
    support of the oracle's output IS the dependency cone.  (Not a numeric impulse: with weights of N(0, 0.02) the
    outermost ring of a 36-layer cone is below fp64 resolution.)  The output pixels whose planned span, clipped to the
    picture, contains the position must equal that support -- too small gives wrong pictures, too large wastes overlap."""
    g = _geometry(name, i)
    make_ora, (h, w) = NETS[name][i][1], NETS[name][i][2]
    ora = make_ora().eval()
    nc = 3 if name in ("EDSR", "SRGAN") else 1
    x0 = fill.rand((1, nc, h, w), 7)
    with torch.no_grad():
        clean = _last(ora(x0))
        assert torch.isfinite(clean).all()
        oh, ow = int(clean.shape[-2]), int(clean.shape[-1])
        assert (oh, ow) == (g.out_size(h), g.out_size(w))
        for py, px in _positions(h, w):
            x = x0.clone()
            x[0, 0, py, px] = float("nan")
            support = torch.isnan(_last(ora(x))).any(dim=1)[0]
            rows = torch.tensor([g.clipped_span(o, h)[0] <= py <= g.clipped_span(o, h)[1] for o in range(oh)])
            cols = torch.tensor([g.clipped_span(o, w)[0] <= px <= g.clipped_span(o, w)[1] for o in range(ow)])
            want = rows[:, None] & cols[None, :]
            assert torch.equal(support, want), "%s depth %d: NaN at (%d, %d): support %d pixels, planned %d; %r" % (
                name, i, py, px, int(support.sum()), int(want.sum()), g)


def test_geometry_follows_the_module_not_the_name():
    pkg, tiling = _pkg()
    M = pkg.models
    a, b = tiling.net_geometry(M.EDSRNet(3, 4, 16)), tiling.net_geometry(M.EDSRNet(3, 4, 2))
    assert a.reach - b.reach == 2 * 14 and a.scale == b.scale == 4      # two 3x3 convs per residual block
    assert tiling.net_geometry(M.ESPCNNet(1, 8, 3)).scale == 3
    assert tiling.net_geometry(M.ESPCNNet(1, 8, 3)).offset == -8 * 3
    assert tiling.net_geometry(M.SRCNNNet(1, 8)).offset == -16
    f = tiling.net_geometry(M.FSRCNNNet(1, 4, 8, 4, 4))
    assert (f.scale, f.offset) == (4, -16) and f.out_size(30) == 4 * (30 - 5) + 4


@pytest.mark.parametrize("D", [3, 16])
def test_drcn_geometry_is_the_hand_derived_one(D):
    """DRCN has no oracle twin: 2 embedding + D recursions + 2 reconstruction layers of 3 x 3, pad 1, plus the input skip."""
    pkg, tiling = _pkg()
    g = tiling.net_geometry(pkg.models.DRCNNet(1, 4, D))
    assert (g.scale, g.offset, g.lo, g.hi) == (1, 0, -(D + 4), D + 4)
    assert g.reach == D + 4 and g.origin == 0


def test_whole_image_modules_are_refused_by_name():
    pkg, tiling = _pkg()
    M, B = pkg.models, pkg.base_networks
    net = M.EDSRNet(3, 4, 3)
    net.residual_layers[1] = B.ResnetBlock(4, norm='instance')
    with pytest.raises(ValueError, match=r"residual_layers\.1.*instance"):
        tiling.net_geometry(net)
    gen = M.SRGANGenerator(3, 4, 2)
    with pytest.raises(ValueError, match=r"residual_layers\.0\.bn.*training"):
        tiling.net_geometry(gen.train())
    tiling.net_geometry(gen.eval())


# ---- plan invariants -------------------------------------------------------------------------------------------------
def _all_geometries():
    pkg, tiling = _pkg()
    out = [("%s-%d" % c, _geometry(*c)) for c in CASES]
    out.append(("DRCN-16", tiling.net_geometry(pkg.models.DRCNNet(1, 4, 16))))
    return out


def _check_axis(tiling, g, n, tile):
    ax = tiling.AxisPlan(g, n, tile)
    T = min(tile, n)
    assert ax.tile == T and ax.n_out == g.out_size(n) and ax.tile_out == g.out_size(T)
    assert ax.starts[0] == 0 and ax.starts[-1] == n - T
    assert all(b > a for a, b in zip(ax.starts, ax.starts[1:]))
    owner = [0] * ax.n_out
    for x, (o0, o1) in zip(ax.starts, ax.own):
        assert 0 <= x and x + T <= n                                  # inside the picture, equal size
        assert 0 <= o0 < o1 <= ax.n_out
        for o in range(o0, o1):
            owner[o] += 1
            q = o - g.scale * x                                       # where the tile computes it
            assert 0 <= q < ax.tile_out
            a, b = g.clipped_span(o, n)
            assert x <= a and b <= x + T - 1, (n, tile, x, o, a, b)   # the clipped cone lies inside the tile
    assert owner == [1] * ax.n_out                                    # owned exactly once
    return ax


def test_plan_invariants_exhaustively():
    _, tiling = _pkg()
    checked = 0
    for name, g in _all_geometries():
        tiles = sorted({g.min_tile, g.min_tile + 1, g.min_tile + 7, 96, 128})
        for tile in tiles:
            extents = sorted({tile - 1, tile, tile + 1, tile + 2, 2 * tile - 1, 97, 131, 157, 211, 2 * tile + 13})
            for n in extents:
                if g.out_size(n) < 1:
                    continue
                _check_axis(tiling, g, n, tile)
                checked += 1
    assert checked > 300


def test_plan_2d_is_the_product_of_its_axes():
    _, tiling = _pkg()
    g = _geometry("EDSR", 0)
    p = tiling.plan(g, 131, 157, 96)
    assert (p.th, p.tw, p.oth, p.otw, p.OH, p.OW) == (96, 96, 384, 384, 524, 628)
    assert len(p.rows) >= 2 and len(p.cols) >= 3 and p.ntiles == len(p.rows) * len(p.cols)
    assert p.rows.starts[-1] == 131 - 96 and p.cols.starts[-1] == 157 - 96        # shifted inwards, not padded
    owned = torch.zeros(p.OH, p.OW, dtype=torch.int32)
    for t, (y0, x0), ((oy0, oy1), (ox0, ox1)) in p.tiles():
        owned[oy0:oy1, ox0:ox1] += 1
    assert int(owned.min()) == 1 and int(owned.max()) == 1
    table = p.table()
    assert len(table) == len(p.rows) + len(p.cols) and all(len(r) == 4 for r in table)
    assert table[len(p.rows) + 1] == [p.cols.starts[1], p.cols.own[1][0], p.cols.own[1][1], 4 * p.cols.starts[1]]
    # extent <= tile: one tile, one pass
    q = tiling.plan(g, 50, 96, 96)
    assert q.ntiles == 1 and (q.th, q.tw) == (50, 96)


def test_pad0_owned_regions_abut_at_the_crop():
    _, tiling = _pkg()
    g = _geometry("SRCNN", 0)
    ax = tiling.AxisPlan(g, 200, 64)
    assert ax.starts[1] - ax.starts[0] == 64 - 16
    assert ax.own[0] == (0, 48) and ax.own[1][0] == 48 == ax.starts[1]     # the crop consumed the overlap


def test_tile_under_the_minimum_is_refused_with_the_minimum():
    _, tiling = _pkg()
    g = _geometry("EDSR", 0)
    assert g.min_tile == 73                    # ceil(2 * 35.75) + 1
    with pytest.raises(ValueError, match="minimum tile is 73"):
        tiling.plan(g, 200, 200, 72)
    tiling.plan(g, 200, 200, 73)
    tiling.plan(g, 60, 60, 72)                 # the picture fits one tile: nothing to overlap
    with pytest.raises(ValueError):
        tiling.plan(g, 200, 200, 0)


def test_auto_budget_is_below_the_kernels_limit():
    _, tiling = _pkg()
    assert 0 < tiling.AUTO_BUDGET_BYTES < 2 ** 31
    g = _geometry("EDSR", 0)                   # 4 channels wide here: 4 * 16 floats per input pixel
    assert tiling.activation_bytes(g, 10, 10) == 4 * 4 * 16 * 100
    assert tiling.resolve_tile(None, g, 100, 100) is None
    assert tiling.resolve_tile("auto", g, 100, 100) is None
    assert tiling.resolve_tile("auto", g, 3000, 3000) == tiling.AUTO_TILE
    assert tiling.resolve_tile(96, g, 100, 100) == 96


# ---- stitching in fp64 -----------------------------------------------------------------------------------------------
SHALLOW = {   # at most 2 residual blocks / 4 body layers, so that 1e-9 separates rounding from an ownership error
    "SRCNN": (lambda M: M.SRCNNNet(1, 8), lambda: R.SRCNN(1, 8), 1, 40),
    "ESPCN": (lambda M: M.ESPCNNet(1, 8, R4), lambda: R.ESPCN(1, 8, R4), 1, 24),
    "FSRCNN": (lambda M: M.FSRCNNNet(1, R4, 8, 4, 4), lambda: R.FSRCNN(1, R4, 8, 4, 4), 1, 32),
    "VDSR": (lambda M: M.VDSRNet(1, 6, 4), lambda: R.VDSR(1, 6, 4), 1, 32),
    "EDSR": (lambda M: M.EDSRNet(3, 6, 2), lambda: R.EDSR(3, 6, 2), 3, 32),
    "LapSRN": (lambda M: M.LapSRNNet(1, 6, 2), lambda: R.LapSRN(1, 6, 2), 1, 32),
    "SRGAN": (lambda M: M.SRGANGenerator(3, 6, 2), lambda: R.Generator(3, 6, 2), 3, 40),
}


@pytest.mark.parametrize("name", sorted(SHALLOW))
def test_stitch_by_the_plan_equals_one_pass_in_fp64(name):
    """Cut by the plan with plain slicing, run the oracle per tile in double, paste the owned rectangles: the one-pass
    output within 1e-9 absolute on outputs of order 1.  Derived: fp64 summation-order differences are of order 1e-13;
    an ownership error at a depth of 4 layers moves a pixel by about 0.02^4 = 1.6e-7 or more."""
    pkg, tiling = _pkg()
    make, make_ora, nc, tile = SHALLOW[name]
    g = tiling.net_geometry(make(pkg.models).eval())
    ora = fill.fill_module(make_ora()).double().eval()
    h, w = 2 * tile + 9, 3 * tile - 5
    x = fill.rand((1, nc, h, w), 21).double()
    p = tiling.plan(g, h, w, tile)
    assert len(p.rows) >= 3 and len(p.cols) >= 3
    with torch.no_grad():
        want = _last(ora(x))
        assert tuple(want.shape[-2:]) == (p.OH, p.OW)
        got = torch.full_like(want, float("nan"))
        for t, (y0, x0), ((oy0, oy1), (ox0, ox1)) in p.tiles():
            out = _last(ora(x[:, :, y0:y0 + p.th, x0:x0 + p.tw]))
            assert tuple(out.shape[-2:]) == (p.oth, p.otw)
            got[:, :, oy0:oy1, ox0:ox1] = out[:, :, oy0 - g.scale * y0:oy1 - g.scale * y0, ox0 - g.scale * x0:ox1 - g.scale * x0]
    err = float((got - want).abs().max())
    print("%s: output magnitude %.3g, stitched vs one pass max abs difference %.3g" % (name, float(want.abs().max()), err))
    assert err < 1e-9


# ---- command line ----------------------------------------------------------------------------------------------------
def test_cli_tile_flag(tmp_path):
    import main as cli
    base = ["--model_name", "EDSR", "--save_dir", str(tmp_path)]
    assert cli.parse_args(base).tile is None
    assert cli.parse_args(base + ["--tile", "96"]).tile == 96
    assert cli.parse_args(base + ["--tile", "auto"]).tile == "auto"
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--tile", "big"])
