"""The RRDB's pieces without a GPU: the host twin of the slice convolution with a scaled output and two scaled skips
(srk_dense_conv_host_ex) against the fp64 restatement of tests/esrgan_ref.py for every epilogue of its table and both
betas, its bit-equality with srk_dense_conv_host where the epilogue is the identity, the slice scheme of ops.rrdb_trunk
run through the host twin, RRDBNet's state_dict table, the refusals and the exported symbols."""
import ctypes

import pytest
import torch

import esrgan_ref as E
import rdn_ref as R

CASES = ["1x1_k3_two", "3x5_k1_wide", "3x5_b160", "7x9_lrelu_res", "7x9_b48"]


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _pkg()._lib.load()


def _p(v):
    return v if (v is None or isinstance(v, ctypes.c_void_p)) else R.fptr(v)


def _host_ex(lib, d, direction, e, A=None, B=None, W=None, bias=None, R1=None, R2=None, y=None, dy=None, add=None, dA=None,
             betaA=0.0, dB=None, betaB=0.0, dW=None, db=None, beta=0.0):
    return lib.srk_dense_conv_host_ex(ctypes.byref(d), direction, _p(A), _p(B), _p(W), _p(bias), _p(R1), _p(R2),
                                      ctypes.byref(e) if e is not None else None, _p(y), _p(dy), _p(add), _p(dA), betaA,
                                      _p(dB), betaB, _p(dW), _p(db), beta)


def _host(lib, d, direction, A=None, B=None, W=None, bias=None, res=None, y=None, dy=None, add=None, dA=None, betaA=0.0,
          dB=None, betaB=0.0, dW=None, db=None, beta=0.0):
    return lib.srk_dense_conv_host(ctypes.byref(d), direction, _p(A), _p(B), _p(W), _p(bias), _p(res), _p(y), _p(dy), _p(add),
                                   _p(dA), betaA, _p(dB), betaB, _p(dW), _p(db), beta)


def _desc(c, **ld):
    n, h, w = c.dims
    return R.desc(_pkg(), n, h, w, c.k, c.ca, c.cb, c.cout, c.act, R.SLOPE, c.terms, **ld)


def _skips(c, has1, has2):
    n, h, w = c.dims
    r1 = R.Buf(n, h, w, c.cout, off=16, width=c.cout + 16, seed=4001) if has1 else None
    r2 = R.Buf(n, h, w, c.cout, off=32, width=c.cout + 48, seed=4002) if has2 else None
    return r1, r2


@pytest.mark.parametrize("epi", sorted(E.EPILOGUES))
@pytest.mark.parametrize("name", CASES)
def test_host_twin_matches_the_restatement(lib, name, epi):
    c = R.case(name)
    s, r1, has1, r2, has2, a1 = E.EPILOGUES[epi]
    R1, R2 = _skips(c, has1, has2)
    e = _pkg()._lib.DenseEpilogue(s, r1, r2, R2.width if R2 else 0, a1)
    a, b = c.A.nchw(), (c.B.nchw() if c.B else None)
    # forward into a NaN-filled slice of a patterned buffer
    Y = c.out_buf(c.cout, 32, c.cout + 48)
    before = Y.t.clone()
    d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldY=Y.width, ldR=R1.width if R1 else 0)
    assert _host_ex(lib, d, 0, e, A=c.A.ptr(), B=c.B.ptr() if c.B else None, W=c.W, bias=c.bias, R1=R1.ptr() if R1 else None,
                    R2=R2.ptr() if R2 else None, y=Y.ptr()) == 0
    want = E.conv_ex_forward(a, b, c.W, c.bias, c.act, s, r1, R1.nchw() if R1 else None, r2, R2.nchw() if R2 else None)
    assert R.worst(Y.nchw(), want) <= 1e-6 and Y.outside_equal(before)          # fp64 accumulation, one rounding
    # data gradient: beta 0 over NaN with the scaled `add`, then beta 1 on top of it
    DA, DB = c.out_buf(c.ca, 16, c.ca + 32), (c.out_buf(c.cb, 48, c.cb + 64) if c.cb else None)
    before_a, before_b = DA.t.clone(), (DB.t.clone() if DB else None)
    d = _desc(c, ldDy=c.DY.width, ldY=c.YS.width, ldDA=DA.width, ldDB=DB.width if DB else 0, ldAdd=c.ADD.width)
    args = dict(W=c.W, y=c.YS.ptr(), dy=c.DY.ptr(), dA=DA.ptr(), dB=DB.ptr() if DB else None)
    add = a1 * c.ADD.nchw().double()
    assert _host_ex(lib, d, 1, e, add=c.ADD.ptr(), betaA=0.0, betaB=0.0, **args) == 0
    assert R.worst(DA.nchw(), s * c.da + add) <= 1e-6 and DA.outside_equal(before_a)
    if DB:
        assert R.worst(DB.nchw(), s * c.db) <= 1e-6 and DB.outside_equal(before_b)
    assert _host_ex(lib, d, 1, e, betaA=1.0, betaB=1.0, **args) == 0
    assert R.worst(DA.nchw(), 2 * s * c.da + add) <= 1e-6 and DA.outside_equal(before_a)
    if DB:
        assert R.worst(DB.nchw(), 2 * s * c.db) <= 1e-6 and DB.outside_equal(before_b)
    # weight gradient: beta 0 over NaN, then beta 1
    dW, db = torch.full_like(c.W, float("nan")), torch.full_like(c.bias, float("nan"))
    d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldDy=c.DY.width, ldY=c.YS.width)
    args = dict(A=c.A.ptr(), B=c.B.ptr() if c.B else None, y=c.YS.ptr(), dy=c.DY.ptr(), dW=dW, db=db)
    assert _host_ex(lib, d, 2, e, beta=0.0, **args) == 0
    assert R.worst(dW, s * c.dw) <= 1e-6 and R.worst(db, s * c.dbias) <= 1e-6
    assert _host_ex(lib, d, 2, e, beta=1.0, **args) == 0
    assert R.worst(dW, 2 * s * c.dw) <= 1e-6 and R.worst(db, 2 * s * c.dbias) <= 1e-6


def test_the_restated_gradient_is_autograds():
    """s * (the plain operator's gradients) is what autograd gives for s * act(conv) -- the table above leans on it."""
    c = R.case("7x9_lrelu_res")
    da, db, dw, dbias = E.conv_ex_grads(c.A.nchw(), c.B.nchw(), c.W, c.bias, c.DY.nchw(), c.act, -1.5)
    assert R.worst(da, -1.5 * c.da) <= 1e-12 and R.worst(db, -1.5 * c.db) <= 1e-12
    assert R.worst(dw, -1.5 * c.dw) <= 1e-12 and R.worst(dbias, -1.5 * c.dbias) <= 1e-12


@pytest.mark.parametrize("with_struct", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_identity_epilogue_gives_the_bits_of_the_plain_twin(lib, name, with_struct):
    c = R.case(name)
    e = _pkg()._lib.DenseEpilogue(1.0, 1.0, 0.0, 0, 1.0) if with_struct else None
    R1, _ = _skips(c, True, False)
    ya, yb = c.out_buf(c.cout, 32, c.cout + 48), c.out_buf(c.cout, 32, c.cout + 48)
    d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldY=ya.width, ldR=R1.width)
    fwd = dict(A=c.A.ptr(), B=c.B.ptr() if c.B else None, W=c.W, bias=c.bias)
    assert _host(lib, d, 0, res=R1.ptr(), y=ya.ptr(), **fwd) == 0
    assert _host_ex(lib, d, 0, e, R1=R1.ptr(), y=yb.ptr(), **fwd) == 0
    assert torch.equal(ya.t.view(torch.int32), yb.t.view(torch.int32))
    outs = []
    for ex in (False, True):
        DA, DB = c.out_buf(c.ca, 16, c.ca + 32, inside=0.5), (c.out_buf(c.cb, 48, c.cb + 64, inside=0.25) if c.cb else None)
        d = _desc(c, ldDy=c.DY.width, ldY=c.YS.width, ldDA=DA.width, ldDB=DB.width if DB else 0, ldAdd=c.ADD.width)
        args = dict(W=c.W, y=c.YS.ptr(), dy=c.DY.ptr(), add=c.ADD.ptr(), dA=DA.ptr(), betaA=1.0, dB=DB.ptr() if DB else None,
                    betaB=0.0)
        assert (_host_ex(lib, d, 1, e, **args) if ex else _host(lib, d, 1, **args)) == 0
        dW, db = torch.full_like(c.W, 0.125), torch.full_like(c.bias, float("nan"))
        d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldDy=c.DY.width, ldY=c.YS.width)
        args = dict(A=c.A.ptr(), B=c.B.ptr() if c.B else None, y=c.YS.ptr(), dy=c.DY.ptr(), dW=dW, db=None, beta=1.0)
        assert (_host_ex(lib, d, 2, e, **args) if ex else _host(lib, d, 2, **args)) == 0
        outs.append((DA.t, DB.t if DB else torch.zeros(1), dW))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_slice_scheme_of_the_trunk_is_the_restatement(lib):
    """The addressing ops.rrdb_trunk uses, run through the host twin: per dense block one growth buffer, conv c reading
    A = the block input and B = growth[.., :(c - 1) G] with LeakyReLU, conv5 reading [A | growth] with s = 0.2 and the
    block input as R1 -- and, in the third block, s = 0.04, r1 = 0.2 and the RRDB's input as R2.  No cat, no scaling and
    no addition outside a convolution."""
    f, g, nb = 16, 32, 2
    n, h, w = 2, 5, 7
    rs = E.RES_SCALE
    blocks = E.make_blocks(f, g, nb, 9)
    x = R.rand((n, f, h, w), 4)
    want = E.trunk_forward(x.double(), E.to64(blocks))
    L = _pkg()._lib
    u1 = x.permute(0, 2, 3, 1).contiguous()
    off = lambda t, c: ctypes.c_void_p(t.data_ptr() + 4 * c)
    for rrdb in blocks:
        u = u1
        for k, p in enumerate(rrdb):
            growth = torch.full((n, h, w, 4 * g), float("nan"))
            for c in range(4):
                dd = R.desc(_pkg(), n, h, w, 3, f, c * g, g, R.ACT_LRELU, ldA=f, ldB=4 * g, ldY=4 * g)
                assert _host(lib, dd, 0, A=u, B=off(growth, 0) if c else None, W=p[2 * c], bias=p[2 * c + 1],
                             y=off(growth, c * g)) == 0
            v = torch.full((n, h, w, f), float("nan"))
            dd = R.desc(_pkg(), n, h, w, 3, f, 4 * g, f, R.ACT_NONE, ldA=f, ldB=4 * g, ldY=f, ldR=f)
            e = L.DenseEpilogue(rs, 1.0) if k < 2 else L.DenseEpilogue(rs * rs, rs, 1.0, f)
            assert _host_ex(lib, dd, 0, e, A=u, B=growth, W=p[8], bias=p[9], R1=u, R2=u1 if k == 2 else None, y=v) == 0
            u = v
        u1 = u
    assert R.worst(u1.permute(0, 3, 1, 2), want) <= 1e-6


def test_restatement_matches_the_fp32_cat_composition():
    blocks = E.make_blocks(16, 16, 2, 7)
    x = R.rand((2, 16, 7, 9), 5)
    got = E.trunk_forward(x, blocks)
    want = E.trunk_forward(x.double(), E.to64(blocks))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 16, 7, 9)
    assert R.worst(got, want) <= 1e-5
    one = E.rrdb_forward(x.double(), E.to64(blocks)[0])
    assert R.worst(one, x.double()) > 1e-3          # the block does something


@pytest.mark.parametrize("nb", [1, 23])
def test_state_dict_table(nb):
    pkg = _pkg()
    net = pkg.RRDBNet(3, nf=64, nb=nb, gc=32, scale_factor=4)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    want = E.state_table(3, 64, nb, 32)
    assert got == want
    assert len(got) == 2 * (6 + 15 * nb)
    assert "body.%d.rdb3.conv5.weight" % (nb - 1) in got and got["body.0.rdb1.conv4.weight"] == (32, 160, 3, 3)
    ref = E.RefRRDBNet(3, 64, nb, 32)
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == want


@pytest.mark.parametrize("kwargs,number", [(dict(scale_factor=3), "3"), (dict(scale_factor=2), "2"), (dict(nf=24), "24"),
                                           (dict(gc=8), "8"), (dict(nf=80), "80"), (dict(gc=96), "96"), (dict(nb=0), "0")])
def test_the_net_refuses_by_number(kwargs, number):
    with pytest.raises(ValueError) as err:
        _pkg().RRDBNet(3, **kwargs)
    assert number in str(err.value)


def test_trunk_refusals_name_the_number():
    ops = _pkg().ops
    x = torch.zeros(1, 24, 4, 4)
    blocks = E.make_blocks(24, 16, 1, 1)
    with pytest.raises(ValueError, match="F = 24"):
        ops.rrdb_trunk(x, blocks)
    with pytest.raises(ValueError, match="G = 80"):
        ops.rrdb_trunk(torch.zeros(1, 16, 4, 4), E.make_blocks(16, 80, 1, 1))
    with pytest.raises(ValueError, match="conv5"):
        bad = E.make_blocks(16, 16, 1, 1)
        bad[0] = (bad[0][0][:8] + (torch.zeros(16, 80, 1, 1), bad[0][0][9]),) + bad[0][1:]
        ops.rrdb_trunk(torch.zeros(1, 16, 4, 4), bad)
    with pytest.raises(ValueError, match="3 RDBs"):
        ops.rrdb_trunk(torch.zeros(1, 16, 4, 4), [E.make_blocks(16, 16, 1, 1)[0][:2]])


def test_epilogue_refusals(lib):
    L = _pkg()._lib
    one = torch.zeros(64)
    d = R.desc(_pkg(), 1, 2, 2, 3, 16, 0, 16, ldA=16, ldY=16, ldR=16)
    e = L.DenseEpilogue(0.2, 1.0, 1.0, 12)
    assert _host_ex(lib, d, 0, e, A=one, W=one, y=one, R2=one) == -1 and "ldR2 = 12" in lib.srk_last_error_string().decode()
    e = L.DenseEpilogue(float("inf"))
    assert _host_ex(lib, d, 0, e, A=one, W=one, y=one) == -1 and "finite" in lib.srk_last_error_string().decode()
    e = L.DenseEpilogue(0.2)
    e.struct_size = 8
    assert _host_ex(lib, d, 0, e, A=one, W=one, y=one) == -1 and "struct_size" in lib.srk_last_error_string().decode()
    assert _host_ex(lib, d, 0, None, A=one, W=one, y=one, R2=one) == -1          # R2 without its scale and stride
    d.Cout = 80
    assert _host_ex(lib, d, 0, L.DenseEpilogue(0.2), A=one, W=one, y=one) == -2 and "80" in lib.srk_last_error_string().decode()


def test_symbols_are_declared_and_exported(lib):
    L = _pkg()._lib
    names = ["srk_dense_conv_%s_ex" % s for s in ("forward", "backward_data", "backward_weight", "host")]
    declared = L.header_symbols()
    for n in names:
        assert n in declared and n in L._PROTOTYPES and hasattr(lib, n), n
    assert lib.srk_version() == 600
    assert ctypes.sizeof(L.DenseEpilogue) == 24 and L.DenseEpilogue().struct_size == 24
    pkg = _pkg()
    for n in ("rrdb_trunk", "ragan_loss", "dense_conv"):
        assert callable(getattr(pkg.ops, n)), n
    assert issubclass(pkg.base_networks.RRDB, torch.nn.Module) and issubclass(pkg.ESRGANDiscriminator, pkg.SRGANDiscriminator)
    assert pkg.ESRGANDiscriminator(3, 16, 32).dense_layers[1].activation is None


def test_perceptual_criterion_is_checked():
    with pytest.raises(ValueError, match="criterion"):
        _pkg().ops.perceptual_loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), None, criterion='huber')


@pytest.mark.parametrize("extra,word", [
    (['--scale_factor', '3', '--vgg_weights', 'v.pth'], '--scale_factor 3'),
    (['--tile', '64', '--vgg_weights', 'v.pth'], '--tile'),
    ([], '--vgg_weights'),
    (['--net_interp', '1.5', '--test_only'], '--net_interp'),
    (['--net_interp', '0.5', '--vgg_weights', 'v.pth'], '--net_interp'),                    # without --test_only
    (['--vgg_weights', 'v.pth', '--ssim_weight', '0.5'], '--ssim_weight'),
    (['--vgg_weights', 'v.pth', '--fft_weight', '0.1'], '--fft_weight'),
    (['--vgg_weights', 'v.pth', '--lpips_weight', '0.1', '--lpips_vgg', 'a', '--lpips_lin', 'b'], '--lpips_weight'),
    (['--vgg_weights', 'v.pth', '--rrdb_growth', '24'], '--rrdb_growth 24'),
    (['--vgg_weights', 'v.pth', '--num_channels', '1'], '--num_channels 1'),
    (['--vgg_weights', 'v.pth', '--gan_weight', '-1'], '--gan_weight'),
], ids=["scale3", "tile", "no_vgg_weights", "interp_1.5", "interp_while_training", "ssim", "fft", "lpips", "growth24", "gray",
        "negative_gan_weight"])
def test_cli_refuses(tmp_path, capsys, extra, word):
    import main
    with pytest.raises(SystemExit):
        main.parse_args(['--save_dir', str(tmp_path / "r"), '--model_name', 'ESRGAN'] + extra)
    assert word in capsys.readouterr().err
    assert not (tmp_path / "r").exists()      # refused at argument checking: nothing was set up


def test_cli_refuses_a_world_above_one(tmp_path, capsys, monkeypatch):
    import main
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        main.parse_args(['--save_dir', str(tmp_path / "r"), '--model_name', 'ESRGAN', '--vgg_weights', 'v.pth'])
    assert 'one GPU' in capsys.readouterr().err


def test_cli_accepts_and_defaults(tmp_path):
    import main
    base = ['--save_dir', str(tmp_path / "r"), '--model_name', 'ESRGAN']
    a = main.parse_args(base + ['--vgg_weights', 'v.pth'])
    assert (a.rrdb_blocks, a.rrdb_growth, a.gan_weight, a.pixel_weight, a.vgg_loss_weight) == (23, 32, 5e-3, 1e-2, 1.0)
    assert a.net_interp is None and a.scale_factor == 4
    a = main.parse_args(base + ['--test_only', '--net_interp', '0.25', '--rrdb_blocks', '2', '--rrdb_growth', '16'])
    assert a.net_interp == 0.25 and (a.rrdb_blocks, a.rrdb_growth) == (2, 16) and a.vgg_weights is None
    assert main.parse_args(base + ['--test_single', 'p.png']).vgg_weights is None
    # another model keeps SRGAN's default weight for the flag, and has no --net_interp
    assert main.parse_args(['--save_dir', str(tmp_path / "r"), '--model_name', 'SRGAN']).vgg_loss_weight == 6e-3


def test_net_interp_belongs_to_esrgan(tmp_path, capsys):
    import main
    with pytest.raises(SystemExit):
        main.parse_args(['--save_dir', str(tmp_path / "r"), '--model_name', 'EDSR', '--test_only', '--net_interp', '0.5'])
    assert '--net_interp' in capsys.readouterr().err


def test_tiling_names_the_rrdb():
    pkg = _pkg()
    net = pkg.RRDBNet(3, nf=16, nb=1, gc=16).eval()
    from pytorch_super_resolution_model_collection_amd import tiling
    with pytest.raises(ValueError, match="body.0: RRDB"):
        tiling.net_geometry(net)


def test_step_builder_checks_its_arguments():
    tr = _pkg().trainers
    with pytest.raises(ValueError, match="feature_extractor"):
        tr.esrgan_segments(None, torch.nn.Linear(1, 1), None, None, None)
    with pytest.raises(ValueError, match="gan_weight"):
        tr.esrgan_segments(None, torch.nn.Linear(1, 1), None, None, object(), gan_weight=-1.0)
    opt = _pkg().optim
    assert "esrgan_g" in open(opt.__file__).read() and "esrgan_d" in open(opt.__file__).read()
