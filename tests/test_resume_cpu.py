"""Host side of --resume / --ema_decay / --use_ema: the library's two new entry points, the command line, the loader's
state, the compatibility check of a training-state file and the file format (plain containers and CPU tensors, readable
with torch.load(weights_only=True)).  No GPU."""
import ctypes

import pytest
import torch

import __graft_entry__


@pytest.fixture(scope="module")
def built():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def test_library_exports_the_ema_entry_points(built):
    lib = built._lib.load()
    for name in ("srk_adam_step_ema", "srk_sgd_step_ema"):
        assert name in built._lib.header_symbols()
        fn = getattr(lib, name)                     # AttributeError: not exported
        assert fn.restype is ctypes.c_int
        plain = getattr(lib, name[:-len("_ema")])
        # the plain entry point's arguments, then `float* ema, float ema_decay` in front of the stream
        assert list(fn.argtypes) == list(plain.argtypes[:-1]) + [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    assert lib.srk_version() == 600


def _parse(tmp_path, *argv):
    import main as cli
    return cli.parse_args(list(argv) + ["--save_dir", str(tmp_path)])


def test_cli_accepts_the_three_flags(tmp_path):
    a = _parse(tmp_path, "--model_name", "ESPCN")
    assert a.resume is None and a.ema_decay == 0.0 and a.use_ema is False
    a = _parse(tmp_path, "--model_name", "ESPCN", "--resume", "--ema_decay", "0.999", "--use_ema")
    assert a.resume == "auto" and a.ema_decay == 0.999 and a.use_ema is True
    a = _parse(tmp_path, "--model_name", "DRCN", "--resume", "some/state.pkl")
    assert a.resume == "some/state.pkl"
    assert _parse(tmp_path, "--model_name", "EDSR", "--ema_decay", "0").ema_decay == 0.0


@pytest.mark.parametrize("argv", [["--ema_decay", "1"], ["--ema_decay", "-0.1"], ["--ema_decay", "nan"],
                                  ["--ema_decay", "0.9", "--model_name", "DRCN"], ["--resume", "--test_only"]])
def test_cli_rejects(tmp_path, argv):
    with pytest.raises(SystemExit):
        _parse(tmp_path, *argv)


class _Stub(object):
    """A dataset as far as PatchLoader._order() needs one."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("world", [1, 2])
def test_patch_loader_state_round_trip(built, world):
    data = built.data
    for rank in range(world):
        whole = data.PatchLoader(_Stub(11), 4, shuffle=True, num_threads=1, seed=1234, rank=rank, world=world)
        first = [whole._order() for _ in range(3)]
        sd = whole.state_dict()
        want = [whole._order() for _ in range(2)]
        assert want[0] != want[1] and want[0] != first[0]
        # a fresh loader (its generator at the seed) continues where the first one stood
        again = data.PatchLoader(_Stub(11), 4, shuffle=True, num_threads=1, seed=1234, rank=rank, world=world)
        again.load_state_dict(sd)
        assert [again._order() for _ in range(2)] == want
        assert not torch.equal(sd["gen"], whole.state_dict()["gen"])   # a snapshot: it did not move with the generator
        for ld in (whole, again):
            ld.pool.shutdown()


def test_compatibility_check_names_the_field(built):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import STATE_VERSION, check_resume_state
    good = {"version": STATE_VERSION, "model_name": "EDSR", "num_channels": 3, "scale_factor": 4}
    check_resume_state(good, "EDSR", 3, 4)
    for field, other in (("model_name", "VDSR"), ("num_channels", 1), ("scale_factor", 2)):
        with pytest.raises(ValueError, match=field):
            check_resume_state(dict(good, **{field: other}), "EDSR", 3, 4)
    with pytest.raises(ValueError, match="version"):
        check_resume_state(dict(good, version=STATE_VERSION + 1), "EDSR", 3, 4)
    with pytest.raises(ValueError, match="version"):
        check_resume_state([1, 2], "EDSR", 3, 4)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_state_file_format_loads_weights_only(built, tmp_path):
    """A state with every kind of member the trainers and optimizers put in (see optim.*.state_dict and
    sr_trainers._Trainer.training_state), built by hand."""
    import random
    from pytorch_super_resolution_model_collection_amd.sr_trainers import STATE_VERSION, check_resume_state
    rnd = random.getstate()
    adam = {"kind": "adam", "hyper": {"betas": [0.9, 0.999], "eps": 1e-8, "weight_decay": 0.0}, "lr": 5e-5, "step": 17,
            "state": {"conv.weight": {"exp_avg": torch.randn(4, 3, 3, 3), "exp_avg_sq": torch.rand(4, 3, 3, 3)},
                      "conv.bias": {"exp_avg": torch.randn(4), "exp_avg_sq": torch.rand(4)}},
            "ema": {"decay": 0.999, "params": {"conv.weight": torch.randn(4, 3, 3, 3), "conv.bias": torch.randn(4)}}}
    sgd = {"kind": "sgd", "hyper": {"momentum": 0.9, "weight_decay": 1e-4, "nesterov": True}, "lr": 1e-6,
           "state": {"fc.weight": {"momentum_buffer": torch.randn(2, 5)}}}
    state = {"version": STATE_VERSION, "model_name": "SRGAN", "num_channels": 3, "scale_factor": 4, "epochs_done": 3,
             "phase": "adversarial", "batch_size": 2, "lr": 1e-4, "world": 1, "history": [[0.5, 0.25], [0.4, 0.2]],
             "modules": {"G": {"conv.weight": torch.randn(4, 3, 3, 3), "bn.num_batches_tracked": torch.tensor(7)},
                         "D": {"fc.weight": torch.randn(2, 5)}},
             "optimizers": {"g_opt": adam, "d_opt": sgd}, "loss_alpha": 0.84,
             "python_random": [rnd[0], list(rnd[1]), rnd[2]], "torch_rng": torch.get_rng_state(),
             "loader": {"gen": torch.Generator().manual_seed(5).get_state()}}
    name = str(tmp_path / "state.pkl")
    torch.save(state, name)
    back = torch.load(name, map_location="cpu", weights_only=True)
    assert _same(state, back)
    check_resume_state(back, "SRGAN", 3, 4)
    r = back["python_random"]
    random.setstate((r[0], tuple(r[1]), r[2]))
    assert random.getstate() == rnd
