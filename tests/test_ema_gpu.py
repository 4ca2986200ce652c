"""The weight EMA fused into the optimizer kernels (srk_adam_step_ema / srk_sgd_step_ema, --ema_decay) on the MI355X:
the entry points against the plain ones (bit for bit) and against fp64, the optimizers (eager and replayed), the EMA
state_dict, and the trainers' ..._ema.pkl files.

Bars.  One EMA update is a subtraction, a multiply and an add in fp32: with m = max(|ema_old|, |p_new|) the three
roundings are at most 2^-24 * (2 m (1 - d) + 2 m (1 - d) + m), within the issue's 2^-22 * m for every decay used here
(d >= 0.5, for which 1.f - d is exact in fp32, so the fp64 formula and the kernel use the same factor).  Over many steps
the per-step rounding is amplified by at most 1 / (1 - d) = 10 at d = 0.9: 10 * 2^-22 * max|p|."""
import numpy as np
import pytest
import torch

from oracle import fill

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -22
B = fill.rand


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _lib():
    pkg = _pkg()
    return pkg._lib.load(), pkg._lib.ptr, pkg._lib.check, pkg._lib.stream_ptr


def _three_trips(gpu):
    """The smallest multiple of 4 floats at which every thread of Adam's 16-byte form (256 threads a block, at most two
    blocks per CU: grid_for(groups, 512, 2 * CUs)) walks its grid-stride loop three times; some walk it a fourth time."""
    blocks = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    return 4 * (3 * blocks * 256 + 5 * 256 + 3)


def _bufs(gpu, n, off, seed, count):
    """`count` independent fp32 device vectors of n floats, each `off` floats past a 256-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        base = torch.empty(n + off + 64, dtype=torch.float32, device=gpu)
        assert base.data_ptr() % 256 == 0
        v = base[off:off + n]
        v.copy_(torch.randn(n, generator=g))
        out.append(v)
    return out


ADAM_CASES = [dict(wd=0.0, d=0.9), dict(wd=1e-2, d=0.999)]
SGD_CASES = [dict(mom=0.0, wd=0.0, nesterov=0, d=0.9), dict(mom=0.9, wd=0.0, nesterov=0, d=0.5),
             dict(mom=0.9, wd=1e-4, nesterov=1, d=0.999)]


def _adam(gpu, n, off, case, lr_dev, ema):
    """One Adam step on seeded buffers through the plain (ema=False) or the EMA entry point -> the buffers afterwards."""
    lib, ptr, check, stream = _lib()
    p, g, m, v, e = _bufs(gpu, n, off, 11, 5)
    m.mul_(0.1)
    v.abs_()
    step = torch.tensor([3, 0], dtype=torch.int32, device=gpu)
    lr = torch.tensor([1e-2], device=gpu) if lr_dev else None
    gs = torch.tensor([0.5], device=gpu)
    e_old = e.clone()
    args = [ptr(p), ptr(g), ptr(m), ptr(v), n, 0.0 if lr_dev else 1e-2, 0.9, 0.999, 1e-8, case["wd"], ptr(step), ptr(lr),
            ptr(gs)]
    if ema:
        check(lib.srk_adam_step_ema(*(args + [ptr(e), case["d"], stream()])), "srk_adam_step_ema")
    else:
        check(lib.srk_adam_step(*(args + [stream()])), "srk_adam_step")
    torch.cuda.synchronize()
    return dict(p=p, m=m, v=v, step=step, ema=e, ema_old=e_old)


def _sgd(gpu, n, off, case, lr_dev, ema):
    lib, ptr, check, stream = _lib()
    p, g, buf, e = _bufs(gpu, n, off, 12, 4)
    lr = torch.tensor([1e-2], device=gpu) if lr_dev else None
    gs = torch.tensor([0.5], device=gpu)
    e_old = e.clone()
    args = [ptr(p), ptr(g), ptr(buf) if case["mom"] else None, n, 0.0 if lr_dev else 1e-2, case["mom"], case["wd"],
            case["nesterov"], 0, ptr(lr), ptr(gs)]
    if ema:
        check(lib.srk_sgd_step_ema(*(args + [ptr(e), case["d"], stream()])), "srk_sgd_step_ema")
    else:
        check(lib.srk_sgd_step(*(args + [stream()])), "srk_sgd_step")
    torch.cuda.synchronize()
    return dict(p=p, buf=buf, ema=e, ema_old=e_old)


def _check_ema(r, d, what):
    """ema within 2^-22 * max(|ema_old|, |p_new|), element-wise, of the fp64 formula on the fp32 p_new."""
    p, e0, e1 = r["p"].double().cpu(), r["ema_old"].double().cpu(), r["ema"].double().cpu()
    one_minus_d = float(np.float32(1.0) - np.float32(d))
    want = e0 + one_minus_d * (p - e0)
    bar = EPS * torch.maximum(e0.abs(), p.abs())
    worst = float(((e1 - want).abs() / bar.clamp_min(1e-300)).max())
    print("%s: worst |ema - fp64| / (2^-22 max(|ema_old|, |p_new|)) = %.3f" % (what, worst))
    assert bool(((e1 - want).abs() <= bar).all()), (what, worst)


# (n, offset in floats): the 4-byte form and its tails, the 16-byte form, a multiple of 4 on misaligned pointers (4-byte
# form), and a size at which the capped grid loops
SIZES = [(1, 0), (3, 0), (4, 0), (5, 0), (1023, 0), (1024, 0), (4100, 0), (1024, 1), ("three_trips", 0)]


@pytest.mark.parametrize("n,off", SIZES, ids=["n%s_off%d" % s for s in SIZES])
def test_entry_points_one_step(gpu, n, off):
    if n == "three_trips":
        n = _three_trips(gpu)
        assert n % 4 == 0 and n // 4 > 3 * 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * 256
    for lr_dev in (True, False):
        for case in ADAM_CASES:
            what = "adam n=%d off=%d lr_dev=%d %s" % (n, off, lr_dev, case)
            plain, fused = _adam(gpu, n, off, case, lr_dev, False), _adam(gpu, n, off, case, lr_dev, True)
            for k in ("p", "m", "v", "step"):
                assert torch.equal(plain[k], fused[k]), (what, k)
            assert fused["step"].tolist() == [4, 0]
            assert torch.equal(plain["ema"], plain["ema_old"])
            _check_ema(fused, case["d"], what)
        for case in SGD_CASES:
            what = "sgd n=%d off=%d lr_dev=%d %s" % (n, off, lr_dev, case)
            plain, fused = _sgd(gpu, n, off, case, lr_dev, False), _sgd(gpu, n, off, case, lr_dev, True)
            for k in ("p", "buf"):
                assert torch.equal(plain[k], fused[k]), (what, k)
            _check_ema(fused, case["d"], what)


def test_entry_points_refuse_bad_arguments(gpu):
    lib, ptr, check, stream = _lib()
    p, g, m, v, e = _bufs(gpu, 8, 0, 13, 5)
    step = torch.zeros(2, dtype=torch.int32, device=gpu)
    before = [t.clone() for t in (p, m, v, e, step)]
    for ema, d in ((None, 0.9), (ptr(e), 1.0), (ptr(e), -0.1), (ptr(e), float("nan"))):
        assert lib.srk_adam_step_ema(ptr(p), ptr(g), ptr(m), ptr(v), 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, ptr(step), None, None,
                                     ema, d, stream()) != 0
        assert lib.srk_sgd_step_ema(ptr(p), ptr(g), ptr(m), 8, 1e-3, 0.9, 0.0, 0, 0, None, None, ema, d, stream()) != 0
    torch.cuda.synchronize()
    for a, b in zip(before, (p, m, v, e, step)):
        assert torch.equal(a, b)     # nothing was launched


@pytest.mark.parametrize("opt_kind,n", [("adam", 4100), ("adam", 1023), ("sgd", 4100), ("sgd", 1023)])
def test_fifty_steps_follow_the_fp64_ema(gpu, opt_kind, n):
    lib, ptr, check, stream = _lib()
    d = 0.9
    one_minus_d = float(np.float32(1.0) - np.float32(d))
    p, m, v = _bufs(gpu, n, 0, 21, 3)
    m.zero_()
    v.zero_()
    e = p.clone()
    step = torch.zeros(2, dtype=torch.int32, device=gpu)
    want = p.double().cpu()
    pmax, worst = float(p.abs().max()), 0.0
    gen = torch.Generator().manual_seed(22)
    for t in range(50):
        g = torch.randn(n, generator=gen).to(gpu)
        if opt_kind == "adam":
            check(lib.srk_adam_step_ema(ptr(p), ptr(g), ptr(m), ptr(v), n, 1e-2, 0.9, 0.999, 1e-8, 0.0, ptr(step), None,
                                        None, ptr(e), d, stream()), "srk_adam_step_ema")
        else:
            check(lib.srk_sgd_step_ema(ptr(p), ptr(g), ptr(m), n, 1e-2, 0.9, 0.0, 0, 0, None, None, ptr(e), d, stream()),
                  "srk_sgd_step_ema")
        pc = p.double().cpu()
        want = want + one_minus_d * (pc - want)
        pmax = max(pmax, float(pc.abs().max()))
        err = float((e.double().cpu() - want).abs().max())
        worst = max(worst, err / (10 * EPS * pmax))
        assert err <= 10 * EPS * pmax, (t, err, pmax)
    print("%s n=%d: worst |ema - fp64 ema| / (10 * 2^-22 * max|p|) over 50 steps = %.4f" % (opt_kind, n, worst))
    if opt_kind == "adam":
        assert step.tolist() == [50, 0]
    assert float((e - p).abs().max()) > 0      # (the shadow lags the parameters: it is not a copy)


def _espcn(gpu, ema_decay, seed=1):
    pkg = _pkg()
    net = pkg.ESPCNNet(3, 64, 4)
    fill.fill_module(net, seed)
    net.to(gpu).train()
    return (net,) + tuple(pkg.trainers.build("espcn", net, 1e-3, ema_decay=ema_decay))


def _espcn_batches(gpu, count):
    return [(B((2, 3, 16, 16), 200 + i).to(gpu), B((2, 3, 32, 32), 300 + i).to(gpu)) for i in range(count)]


def test_optimizer_without_ema_allocates_nothing_and_calls_the_old_symbol(gpu, monkeypatch):
    pkg = _pkg()
    net, flat, opt, dp, step = _espcn(gpu, 0.0)
    assert opt.ema is None and opt.ema_decay == 0.0
    lib = pkg._lib.load()
    called = []
    plain = lib.srk_adam_step

    def boom(*a):
        raise AssertionError("the EMA entry point was called with ema_decay == 0")

    def counted(*a):
        called.append(1)
        return plain(*a)

    monkeypatch.setattr(lib, "srk_adam_step_ema", boom)
    monkeypatch.setattr(lib, "srk_adam_step", counted)
    for b in _espcn_batches(gpu, 2):
        step(*b)
    torch.cuda.synchronize()
    assert len(called) == 2
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_state_dict(net)
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            pkg.optim.Adam(flat, 1e-3, ema_decay=bad)


def test_eager_and_replayed_steps_advance_the_shadow_alike(gpu):
    pkg = _pkg()
    d = 0.9
    one_minus_d = float(np.float32(1.0) - np.float32(d))
    net, flat, opt, dp, step = _espcn(gpu, d)
    assert opt.ema is not None and opt.ema.shape == flat.data.shape and opt.ema.data_ptr() % 16 == 0
    assert torch.equal(opt.ema, flat.data)            # initialised to a copy of the parameters
    shadow_ptr = opt.ema.data_ptr()
    batches = _espcn_batches(gpu, 6)
    want, pmax = flat.data.double().cpu(), float(flat.data.abs().max())

    def observe(what):
        nonlocal want, pmax
        pc = flat.data.double().cpu()
        want = want + one_minus_d * (pc - want)
        pmax = max(pmax, float(pc.abs().max()))
        err = float((opt.ema.double().cpu() - want).abs().max())
        print("%s: |ema - fp64 ema| = %.3e, bar %.3e" % (what, err, 10 * EPS * pmax))
        assert err <= 10 * EPS * pmax, what

    for i in range(2):
        step(*batches[i])
        observe("eager step %d" % i)
    before = flat.data.clone()
    graph = pkg.trainers.capture_step(step, batches[2], warmup=0, flats=[flat])
    torch.cuda.synchronize()
    assert torch.equal(before, flat.data)             # (a capture runs nothing)
    for i in range(2, 6):
        graph(*batches[i])
        observe("replayed step %d" % i)
    graph.close()
    assert opt.ema.data_ptr() == shadow_ptr
    assert float((opt.ema - flat.data).abs().max()) > 0
    # ema_reset: the shadow is the parameters again, in the same buffer
    opt.ema_reset()
    assert torch.equal(opt.ema, flat.data) and opt.ema.data_ptr() == shadow_ptr


def test_ema_state_dict_has_the_models_keys_and_shapes(gpu):
    net, flat, opt, dp, step = _espcn(gpu, 0.9)
    for b in _espcn_batches(gpu, 2):
        step(*b)
    sd, esd = net.state_dict(), opt.ema_state_dict(net)
    assert list(sd) == list(esd)
    views = opt._views(opt.ema)
    for k in sd:
        assert esd[k].shape == sd[k].shape and esd[k].dtype == sd[k].dtype
        assert torch.equal(esd[k], views[k])
        assert not torch.equal(esd[k], sd[k]), k       # the shadow, not the live value


def test_ema_state_dict_resolves_shared_parameters_by_identity(gpu):
    """LapSRN's convt_F1 and convt_F2 are two Sequentials over the same blocks: state_dict() has both sets of keys,
    FlatParams.names only the first."""
    pkg = _pkg()
    net = pkg.LapSRNNet(3, 64, 2)
    fill.fill_module(net, 4)
    net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build("lapsrn", net, 1e-3, ema_decay=0.9)
    step(B((2, 3, 8, 8), 90).to(gpu), B((2, 3, 16, 16), 100).to(gpu), B((2, 3, 32, 32), 110).to(gpu))
    sd, esd = net.state_dict(), opt.ema_state_dict(net)
    assert list(sd) == list(esd)
    f2 = [k for k in sd if k.startswith("convt_F2.")]
    assert f2 and not any(k in flat.names for k in f2)
    for k in f2:
        k1 = "convt_F1." + k[len("convt_F2."):]
        assert torch.equal(esd[k], esd[k1]) and esd[k].shape == sd[k].shape
    assert any(not torch.equal(esd[k], sd[k]) for k in f2)


def _train_espcn(tmp_path, ema_decay):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    args = cli.parse_args(["--model_name", "ESPCN", "--synthetic", "--steps_per_epoch", "3", "--num_epochs", "2",
                           "--batch_size", "2", "--crop_size", "64", "--ema_decay", str(ema_decay), "--lr", "1e-3",
                           "--save_dir", str(tmp_path)])
    torch.manual_seed(0)
    t = TRAINERS["ESPCN"](args)
    t.train()
    return t, args


def test_trainer_writes_and_loads_the_ema_file(gpu, tmp_path):
    import os
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    t, args = _train_espcn(tmp_path, 0.9)
    plain_name = os.path.join(str(tmp_path), "ESPCN", "model", "ESPCN_param.pkl")
    ema_name = os.path.join(str(tmp_path), "ESPCN", "model", "ESPCN_param_ema.pkl")
    assert os.path.exists(plain_name) and os.path.exists(ema_name)
    plain, ema = torch.load(plain_name, weights_only=True), torch.load(ema_name, weights_only=True)
    assert list(plain) == list(ema)
    for k in plain:
        assert plain[k].shape == ema[k].shape
        assert not torch.equal(plain[k], ema[k]), k
    # load_model() with use_ema puts the EMA values into the model
    args.use_ema = True
    t2 = TRAINERS["ESPCN"](args)
    t2.model = t2.build_model().to(t2.device)
    assert t2.load_model() is True
    for k, v in t2.model.state_dict().items():
        assert torch.equal(v.cpu(), ema[k]), k
    # ... and says so when the file is missing
    os.remove(ema_name)
    assert t2.load_model() is False


def test_trainer_without_ema_writes_no_ema_file(gpu, tmp_path):
    import os
    _train_espcn(tmp_path, 0)
    files = sorted(os.listdir(os.path.join(str(tmp_path), "ESPCN", "model")))
    assert "ESPCN_param.pkl" in files and not [f for f in files if "_ema" in f], files
