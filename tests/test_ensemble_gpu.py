"""The x8 geometric self-ensemble on the GPU: the two kernels of csrc/dihedral.hip against the definition written with
torch.rot90 / torch.flip (tests/ensemble_ref.py), and test_single / test with self_ensemble=True, one pass and tiled,
against the ensemble of the REFERENCE nets on the CPU."""
import numpy as np
import pytest
import torch
from PIL import Image

import ensemble_ref as E
from oracle import fill, img_interp as O
from test_tile_gpu import (BIG, MODELS, SCALE, SMALL, TOL_FWD, _awkward, _picture, _reference_input, _reference_tail,
                           _trainer)

pytestmark = pytest.mark.gpu

# off the 16-pixel run and off the 32-pixel LDS tile in both axes, thinner and wider strips than a tile, one square
SHAPES = [(45, 67), (33, 16), (17, 250), (1, 19), (48, 48)]


def _ops():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg.ops


def _tiling():
    from pytorch_super_resolution_model_collection_amd import tiling
    return tiling


def _layouts(x, gpu):
    """the same [N,C,H,W] values behind three kinds of strides (the idea of test_tile_gpu._layouts, for a batch)"""
    n, c, h, w = x.shape
    planar = x.to(gpu)
    cl = x.permute(0, 2, 3, 1).contiguous().to(gpu).permute(0, 3, 1, 2)
    big = torch.zeros(n, c, h + 3, w + 9)
    big[:, :, 2:2 + h, 5:5 + w] = x
    strided = big.to(gpu)[:, :, 2:2 + h, 5:5 + w]
    assert (n * c * h == 1 or not strided.is_contiguous()) and (c == 1 or not cl.is_contiguous())   # (one row IS dense)
    return {"planar": planar, "channels_last": cl, "row_strided": strided}


# ---- kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_variants_are_the_rot90_flip_definition(gpu, hw, c):
    ops = _ops()
    h, w = hw
    for n in (1, 2):
        x = fill.randn((n, c, h, w), 5 + h + c + n)
        want = [E.transform(x, k) for k in range(8)]
        for name, src in _layouts(x, gpu).items():
            var = ops.dihedral_variants(src)
            even, odd = var
            assert tuple(even.shape) == (4 * n, c, h, w) and tuple(odd.shape) == (4 * n, c, w, h), name
            base = even.untyped_storage().data_ptr()
            assert odd.untyped_storage().data_ptr() == base                      # views of one allocation
            assert even.permute(0, 2, 3, 1).is_contiguous() and odd.permute(0, 2, 3, 1).is_contiguous()   # channels-last
            ev, od = even.cpu(), odd.cpu()
            for i in range(n):
                for j in range(4):
                    assert torch.equal(ev[4 * i + j], want[2 * j][i]), (name, n, 2 * j)
                    assert torch.equal(od[4 * i + j], want[2 * j + 1][i]), (name, n, 2 * j + 1)
            if h == w:
                assert var.whole is not None and tuple(var.whole.shape) == (8 * n, c, h, h)
                assert var.whole.untyped_storage().data_ptr() == base
                assert torch.equal(var.whole.cpu(), torch.cat([ev, od]))
            else:
                assert var.whole is None
    if c == 1:   # a [C,H,W] picture is a batch of one
        assert torch.equal(ops.dihedral_variants(x[0].to(gpu))[0].cpu(), ev[:4])


def _net_outputs(n, c, oh, ow, seed, make=fill.randn):
    """what a net would return for the eight variants of n pictures: [f(T_k x)] with the shapes of T_k"""
    return [make((n, c, oh, ow) if k % 2 == 0 else (n, c, ow, oh), seed + k) for k in range(8)]


def _definition_on_device(outs, gpu):
    """E from the eight outputs, evaluated with torch ops in fp32 on the device: seven adds in order, then * 0.125"""
    return E.mean_in_order([E.inverse(y.to(gpu), k) for k, y in enumerate(outs)])


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_merge_f32_is_bit_equal_to_the_definition(gpu, hw, c):
    ops = _ops()
    oh, ow = hw
    for n in (1, 2):
        outs = _net_outputs(n, c, oh, ow, 100 + oh + c + n)
        want = _definition_on_device(outs, gpu)
        even, odd = (g.to(gpu) for g in E.groups(outs))
        for layout in ("nchw", "channels_last"):
            if layout == "channels_last":
                even, odd = (g.contiguous(memory_format=torch.channels_last) for g in (even, odd))
            got = ops.dihedral_merge(even, odd)
            assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want), (n, layout)
            out = torch.full((n, c, oh, ow), float("nan"), device=gpu)
            assert ops.dihedral_merge(even, odd, out=out) is out and torch.equal(out, want), (n, layout)


def test_merge_of_the_variants_of_a_picture_is_the_picture(gpu):
    """both kernels end to end with the identity as the net: each y_k is x itself, so E is the ordered sum of eight
    copies of x (3 x, 5 x, ... round in fp32, so that is not x itself), times 0.125"""
    ops = _ops()
    for c, (h, w) in ((3, (45, 67)), (1, (48, 48))):
        x = fill.randn((2, c, h, w), 9).to(gpu)
        want = E.mean_in_order([x] * 8)
        assert float((want - x).abs().max()) < 1e-6
        var = ops.dihedral_variants(x)
        assert torch.equal(ops.dihedral_merge(var.even, var.odd), want)
        if var.whole is not None:
            assert torch.equal(ops.dihedral_merge(var.whole[:8], var.whole[8:]), want)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c", [1, 3])
def test_merge_u8_is_bit_equal_to_the_two_launch_tail(gpu, c, layout):
    ops = _ops()
    oh, ow = 131, 157
    assert ow % 16 and (3 * ow) % 16
    outs = _net_outputs(1, c, oh, ow, 300 + c, make=_awkward)
    even, odd = (g.to(gpu) for g in E.groups(outs))
    if layout == "channels_last":
        even, odd = (g.contiguous(memory_format=torch.channels_last) for g in (even, odd))
    mean = ops.dihedral_merge(even, odd)
    assert bool(torch.isnan(mean).any()) and float(mean.nan_to_num().min()) < 0 and float(mean.nan_to_num().max()) > 1
    assert torch.equal(ops.dihedral_merge_u8(even, odd), ops.to_u8_image(mean))
    if c == 1:
        cbcr = torch.from_numpy(np.random.RandomState(9).randint(0, 256, size=(2, oh, ow), dtype=np.uint8)).to(gpu)
        got = ops.dihedral_merge_u8(even, odd, cb=cbcr[0], cr=cbcr[1])
        assert tuple(got.shape) == (oh, ow, 3) and torch.equal(got, ops.ycbcr_to_rgb_u8(mean, cbcr[0], cbcr[1]))


def test_dihedral_ops_reject_what_they_do_not_cover(gpu):
    ops = _ops()
    z = lambda *s, **kw: torch.zeros(*s, device=gpu, **kw)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError):
        ops.dihedral_variants(torch.zeros(1, 3, 8, 8))                            # host tensor
    with pytest.raises(RuntimeError):
        ops.dihedral_variants(z(1, 2, 8, 8))                                      # C must be 1 or 3
    with pytest.raises(RuntimeError):
        ops.dihedral_variants(z(1, 3, 8, 8, dtype=torch.float16))                 # fp32 only
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(torch.zeros(4, 1, 8, 6), torch.zeros(4, 1, 6, 8))      # host tensors
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(4, 2, 8, 6), z(4, 2, 6, 8))                          # C must be 1 or 3
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(4, 1, 8, 6), z(4, 1, 8, 6))                          # odd is not the transposed shape
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(4, 1, 8, 6), z(8, 1, 6, 8))                          # group sizes differ
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(3, 1, 8, 6), z(3, 1, 6, 8))                          # not whole groups of four
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(4, 1, 8, 6, dtype=torch.float64), z(4, 1, 6, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.dihedral_merge(z(4, 1, 8, 6), z(4, 1, 6, 8), out=z(1, 1, 6, 8))       # out of another shape
    with pytest.raises(RuntimeError):
        ops.dihedral_merge_u8(z(8, 1, 8, 6), z(8, 1, 6, 8))                       # one picture only
    with pytest.raises(RuntimeError):
        ops.dihedral_merge_u8(z(4, 1, 8, 6), z(4, 1, 6, 8), cb=u8(8, 6))          # cb without cr
    with pytest.raises(RuntimeError):
        ops.dihedral_merge_u8(z(4, 3, 8, 6), z(4, 3, 6, 8), cb=u8(8, 6), cr=u8(8, 6))   # chroma with C = 3
    with pytest.raises(RuntimeError):
        ops.dihedral_merge_u8(z(4, 1, 8, 6), z(4, 1, 6, 8), cb=u8(6, 8), cr=u8(6, 8))   # chroma of another size
    with pytest.raises(RuntimeError):
        ops.dihedral_merge_u8(z(4, 1, 8, 6), z(4, 1, 6, 8), cb=z(8, 6), cr=z(8, 6))     # chroma must be 8-bit


# ---- nets, against the ensemble of the reference nets ----------------------------------------------------------------
_ORACLE = {}   # (name, hw) -> the oracle's side of a case, computed once and shared by the tests that need it


def _case(name, hw, tmp_path):
    """The seeded picture of test_tile_gpu at `hw` as the reference feeds it to the net, and the oracle ensemble of it:
    x, chroma, the terms' largest magnitude (the scale of the bar) and E."""
    fn = _picture(tmp_path, hw)
    if (name, hw) not in _ORACLE:
        ora = MODELS[name][1]().eval()
        x, chroma = _reference_input(fn, MODELS[name][0])
        with torch.no_grad():
            xin = O.img_interp(x, SCALE, "bicubic") if name in ("VDSR", "SRCNN") else x
        ys = E.terms(ora, xin)
        _ORACLE[(name, hw)] = (x, chroma, max(float(y.abs().max()) for y in ys), E.mean_in_order(ys), xin, ora)
    return (fn,) + _ORACLE[(name, hw)]


def _within_bar(got, want, scale, what):
    """Derived: the error of a mean is at most the largest error of its terms, and a term is one forward, held to
    TOL_FWD relative to its own magnitude: max |got - want| <= TOL_FWD * max_k max |y_k|."""
    err = float((got.double() - want.double()).abs().max())
    print("%s: max abs error %.3e, bar %.3e (terms up to %.3g)" % (what, err, TOL_FWD * scale, scale))
    assert got.shape == want.shape and err <= TOL_FWD * scale, what


ONE_PASS = {"ESPCN": (45, 67), "FSRCNN": (45, 67), "EDSR": (45, 67), "LapSRN": (45, 67), "SRGAN": (45, 67),
            "VDSR": (17, 23), "SRCNN": (17, 23)}


@pytest.mark.parametrize("name", sorted(ONE_PASS))
def test_single_ensemble_one_pass(gpu, tmp_path, name):
    t, _ = _trainer(name, tmp_path)
    fn, x, chroma, scale, want, xin, ora = _case(name, ONE_PASS[name], tmp_path)
    # every variant on its own first: what the net returns for T_k(x) against the oracle on T_k(x)
    even, odd = t._infer_variants(t._net_input(x.to(gpu)))
    for k in range(8):
        with torch.no_grad():
            ref = ora(E.transform(xin, k).contiguous())
        ref = ref[-1] if isinstance(ref, tuple) else ref
        mine = (odd if k % 2 else even)[k // 2:k // 2 + 1].cpu()
        print("   %s variant %d: max abs error %.3e of %.3g" % (name, k, float((mine - ref).abs().max()), float(ref.abs().max())))
    got = t.test_single(x, self_ensemble=True)
    assert torch.is_tensor(got) and not got.is_cuda
    _within_bar(got, want, scale, "%s one pass" % name)
    assert torch.equal(t.test_single(x[0], self_ensemble=True), got)

    # off means off: False / None are the plain forward of today; the option of the command line equals the keyword
    with torch.no_grad():
        plain = t._infer(t._net_input(x.to(gpu)))
    plain = (plain[-1] if isinstance(plain, tuple) else plain).cpu()
    assert torch.equal(t.test_single(x, self_ensemble=False), plain) and torch.equal(t.test_single(x), plain)
    assert not torch.equal(got, plain)
    t.args.self_ensemble = True
    assert torch.equal(t.test_single(x), got) and torch.equal(t.test_single(x, self_ensemble=False), plain)
    t.args.self_ensemble = False


TILED = {"FSRCNN": (BIG, 64), "EDSR": (BIG, 96)}


@pytest.mark.parametrize("name", sorted(TILED))
def test_single_ensemble_tiled(gpu, tmp_path, name):
    tiling = _tiling()
    hw, tile = TILED[name]
    t, _ = _trainer(name, tmp_path)
    fn, x, chroma, scale, want, xin, _ = _case(name, hw, tmp_path)
    geo = tiling.ensemble_geometry(tiling.net_geometry(t.model))
    plan = tiling.plan(geo, hw[0], hw[1], tile)
    assert len(plan.rows) >= 2 and len(plan.cols) >= 3
    assert plan.rows.starts[-1] == plan.H - plan.th and plan.cols.starts[-1] == plan.W - plan.tw   # shifted inwards
    got = t.test_single(x, tile=tile, self_ensemble=True)
    _within_bar(got, want, scale, "%s tile=%d (%d x %d tiles)" % (name, tile, len(plan.rows), len(plan.cols)))
    for tb in (1, 5, "all"):
        _within_bar(t.test_single(x, tile=tile, tile_batch=tb, self_ensemble=True), want, scale, "   tile_batch=%s" % tb)
    # chunks of two tiles with t0 > 0 and, for an odd count of tiles, a shorter last chunk (16 net inputs = 2 tiles)
    assert _tiling().tiles_per_chunk(16, plan.ntiles, True) == 2 and (name != "FSRCNN" or plan.ntiles % 2 == 1)
    _within_bar(t.test_single(x, tile=tile, tile_batch=16, self_ensemble=True), want, scale, "   tile_batch=16")


PATH = {"EDSR": (BIG, 96), "ESPCN": (BIG, 64), "VDSR": (SMALL, 96)}


@pytest.mark.parametrize("name", sorted(PATH))
def test_single_ensemble_path_form(gpu, tmp_path, name):
    hw, tile = PATH[name]
    t, _ = _trainer(name, tmp_path)
    fn, x, chroma, scale, want, xin, _ = _case(name, hw, tmp_path)
    chain = _reference_tail(want, chroma)               # the whole chain on the CPU with the oracle
    for kw in ({}, {"tile": tile}):
        got = t.test_single(x, self_ensemble=True, **kw)
        _within_bar(got, want, scale, "%s %s tensor form" % (name, kw))
        png = np.asarray(Image.open(t.test_single(fn, self_ensemble=True, **kw))).copy()
        tail = _reference_tail(got, chroma)             # the reference's Pillow tail on the tensor form's output
        print("%s %s exact tail: %d of %d bytes differ" % (name, kw, int((png != tail).sum()), tail.size))
        assert np.array_equal(png, tail)
        diff = np.abs(png.astype(np.int16) - chain.astype(np.int16))
        print("%s %s whole chain: max byte difference %d, %d of %d bytes differ" % (name, kw, int(diff.max()),
                                                                                 int((diff > 0).sum()), diff.size))
        assert png.shape == chain.shape and int(diff.max()) <= 1


def test_test_with_self_ensemble_reports_the_psnr_of_the_ensemble_outputs(gpu, tmp_path):
    import pytorch_super_resolution_model_collection_amd as pkg
    t, _ = _trainer("ESPCN", tmp_path)
    loader, want = [], []
    for i in range(2):
        lr = fill.rand((1, 1, 29 + i, 35), 40 + i)
        hr = fill.rand((1, 1, SCALE * (29 + i - 8), SCALE * (35 - 8)), 50 + i)
        loader.append((lr, hr))
        want.append(float(pkg.utils.PSNR(t.test_single(lr, self_ensemble=True).to(gpu), hr.to(gpu))))
    plain = t.test(loader)
    got = t.test(loader, self_ensemble=True)
    print("test(self_ensemble=True): %s, from the tensor form %s, without %s" % (got, want, plain))
    assert got == want and got != plain


def test_ensemble_paths_do_not_synchronise(gpu, tmp_path):
    """Between the upload and the final copy nothing waits for the device: with torch's synchronisation debugging set
    to raise, the one-pass and the tiled ensemble (fp32) and the 8-bit merge with resized chroma run through."""
    ops, tiling = _ops(), _tiling()
    t, _ = _trainer("ESPCN", tmp_path)
    rgb = torch.from_numpy(np.array(Image.open(_picture(tmp_path, BIG)))).to(gpu)

    def run():
        y, cbcr = ops.rgb_to_ycc_planes(rgb, y_float=True)
        x = y.view(1, 1, *BIG)
        one = t._forward(x, self_ensemble=True)
        tiled = t._forward(x, 64, 8, self_ensemble=True)
        even, odd = t._infer_variants(x)
        cbcr = ops.resize_u8(cbcr, int(even.shape[-2]), int(even.shape[-1]))
        return one, tiled, ops.dihedral_merge_u8(even, odd, cbcr[0], cbcr[1])
    want = run()   # warm: the first launch of a net packs its filters
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
