"""VESPCN without a GPU: the flag rules of sr_trainers.VESPCN, the net's state_dict keys and shapes, its size rules, the
output geometry of the fp64 restatement (tests/vespcn_ref.py) and the restated warp against tests/mc_ref.py."""
import argparse
import os

import numpy as np
import pytest
import torch

import __graft_entry__
import mc_ref
import vespcn_ref as V


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    from pytorch_super_resolution_model_collection_amd import models, sr_trainers, tiling, utils, video_stream   # noqa: F401
    return p


def ns(**kw):
    base = dict(model_name="VESPCN", crop_size=128, scale_factor=4, num_channels=3, synthetic=True)
    base.update(kw)
    return argparse.Namespace(**base)


def test_refusals_name_the_flag(pkg, monkeypatch):
    T = dict(pkg.sr_trainers.TRAINERS, **pkg.sr_trainers.VIDEO_TRAINERS)
    assert "VESPCN" not in pkg.sr_trainers.TRAINERS and pkg.sr_trainers.trainer_class("VESPCN").kind == "vespcn"
    assert pkg.sr_trainers.model_names() == list(pkg.sr_trainers.TRAINERS) + ["VESPCN"]
    assert pkg.sr_trainers.trainer_class("ESPCN") is pkg.sr_trainers.ESPCN
    check = T["VESPCN"].check_flags
    check(ns())
    check(ns(mc_weight=0.5, flow_weight=0.0, vespcn_max_flow=4.0))
    for kw, word in ((dict(tile=16), "--tile"), (dict(tile="auto"), "--tile"), (dict(self_ensemble=True), "--self_ensemble"),
                     (dict(degrade=True, synthetic=False), "--degrade"), (dict(degrade_test=(1, 1, 0, 0), synthetic=False), "--degrade_test"),
                     (dict(degrade2={}, synthetic=False), "--degrade2"), (dict(degrade2_test=3, synthetic=False), "--degrade2_test"),
                     (dict(usm=True, synthetic=False), "--usm"), (dict(jpeg_quality=(30, 90), synthetic=False), "--jpeg_quality"),
                     (dict(jpeg_test=50, synthetic=False), "--jpeg_test"), (dict(ssim_weight=0.1), "--ssim_weight"),
                     (dict(fft_weight=0.1), "--fft_weight"), (dict(lpips_weight=0.1), "--lpips_weight"),
                     (dict(vespcn_max_flow=0.0), "--vespcn_max_flow"), (dict(crop_size=40), "--crop_size 40"),
                     (dict(crop_size=30, scale_factor=3), "--crop_size 30")):
        with pytest.raises(ValueError, match=word):
            check(ns(**kw))
    check(ns(crop_size=36, scale_factor=3, tile=None, self_ensemble=False, ssim_weight=0.0))   # 12 is a multiple of 4
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="VESPCN trains on one GPU"):
        check(ns())
    monkeypatch.delenv("WORLD_SIZE")
    for other in ("ESPCN", "EDSR", "SRGAN"):
        for flag in ("mc_weight", "flow_weight", "vespcn_max_flow"):
            with pytest.raises(ValueError, match="--%s: only VESPCN" % flag):
                T[other].check_flags(ns(model_name=other, **{flag: 0.5}))
        T[other].check_flags(ns(model_name=other, mc_weight=None))


def test_main_relays_the_rules(pkg, capsys):
    import main
    args = main.parse_args(["--model_name", "VESPCN", "--synthetic", "--crop_size", "64"])
    assert args.mc_weight is None and args.flow_weight is None and args.vespcn_max_flow is None
    assert pkg.sr_trainers.VESPCN.hyper(args) == {"mc_weight": 0.01, "flow_weight": 0.001, "vespcn_max_flow": 8.0}
    for argv, word in ((["--model_name", "ESPCN", "--mc_weight", "0.1"], "--mc_weight: only VESPCN"),
                       (["--model_name", "VESPCN", "--crop_size", "40"], "not a multiple of 4"),
                       (["--model_name", "VESPCN", "--tile", "16"], "--tile: VESPCN")):
        with pytest.raises(SystemExit):
            main.parse_args(argv + ["--synthetic"])
        assert word in capsys.readouterr().err


def test_state_dict_keys_and_shapes(pkg):
    for c, r in ((1, 2), (3, 3), (3, 4)):
        net = pkg.models.VESPCNNet(c, 64, r, 8.0)
        want = {}
        for i, (co, ci, k) in enumerate([(24, 2 * c, 5), (24, 24, 3), (24, 24, 5), (24, 24, 3), (32, 24, 3)]):
            want["mc.coarse.%d.conv.weight" % i], want["mc.coarse.%d.conv.bias" % i] = (co, ci, k, k), (co,)
        for i, (co, ci, k) in enumerate([(24, 3 * c + 2, 5), (24, 24, 3), (24, 24, 3), (24, 24, 3), (8, 24, 3)]):
            want["mc.fine.%d.conv.weight" % i], want["mc.fine.%d.conv.bias" % i] = (co, ci, k, k), (co,)
        for i, (co, ci, k) in enumerate([(64, 3 * c, 5), (32, 64, 3), (c * r * r, 32, 3)]):
            want["layers.%d.conv.weight" % i], want["layers.%d.conv.bias" % i] = (co, ci, k, k), (co,)
        got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert got == want
    with pytest.raises(ValueError, match="max_flow 0 is not positive"):
        pkg.models.VESPCNNet(1, 64, 2, 0)


def test_size_rules(pkg):
    net = pkg.models.VESPCNNet(1, 64, 2)
    x = torch.arange(3 * 18 * 22, dtype=torch.float32).reshape(1, 3, 1, 18, 22)
    net.train()
    with pytest.raises(ValueError, match="18 x 22 input is not a multiple of 4"):
        net.check_image_size(x)
    assert net.check_image_size(x[..., :16, :20]) is not None
    net.eval()
    padded = net.check_image_size(x)
    assert tuple(padded.shape) == (1, 3, 1, 20, 24) and torch.equal(padded, V.pad4(x))
    with pytest.raises(ValueError, match=r"expects \[N,3,1,H,W\]"):
        net.check_image_size(x[:, :2])
    with pytest.raises(ValueError, match="leaves nothing"):
        net.check_image_size(x[..., :8, :8])
    with pytest.raises(ValueError, match="not a multiple of 4"):
        net.mc(torch.zeros(2, 2, 10, 12))
    with pytest.raises(ValueError, match="MotionCompensator"):
        pkg.tiling.net_geometry(net)


def test_reference_geometry_and_warp():
    torch.manual_seed(0)
    import pytorch_super_resolution_model_collection_amd as p
    for c, r, h, w in ((1, 2, 16, 16), (3, 3, 12, 20)):
        net = p.models.VESPCNNet(c, 64, r)
        sd = {k: v.double() for k, v in net.state_dict().items()}
        sr, mc, flow, coarse = V.forward_terms(sd, torch.rand(2, 3, c, h, w, dtype=torch.float64), r)
        assert tuple(sr.shape) == (2, c, r * (h - 8), r * (w - 8)) and tuple(flow.shape) == (4, 2, h, w) and mc.shape == ()
        assert float(flow.abs().max()) <= 8.0 * 1.25
    # the restated warp and its written-out masks against the numpy yardstick, on the integers and the bounds too
    for shape, family in mc_ref.cases():
        frames, flow = mc_ref.case(shape, family)
        n = shape[0]
        g = np.random.RandomState(2).randn(n, shape[1], shape[2], shape[3])
        want, want_d = mc_ref.warp(frames[:, 0], flow[:n], g)
        fl = torch.from_numpy(flow[:n]).double().requires_grad_(True)
        out = V.warp(torch.from_numpy(frames[:, 0]).double(), fl)
        (out * torch.from_numpy(g)).sum().backward()
        assert np.abs(out.detach().numpy() - want).max() <= 1e-12 and np.abs(fl.grad.numpy() - want_d).max() <= 1e-12
        lw, lg = mc_ref.flow_huber(flow)
        fl = torch.from_numpy(flow).double().requires_grad_(True)
        t = V.flow_huber(fl)
        t.backward()
        assert abs(float(t.detach()) - lw) <= 1e-12 and np.abs(fl.grad.numpy() - lg).max() <= 1e-12


def test_synthetic_batches(pkg):
    args = argparse.Namespace(batch_size=2, num_channels=1, scale_factor=2, crop_size=32)
    frames, hr = next(pkg.sr_trainers.synthetic_loader("vespcn", args, 1, "cpu"))
    assert tuple(frames.shape) == (2, 3, 1, 16, 16) and tuple(hr.shape) == (2, 1, 32, 32)
    assert tuple(pkg.utils.shave(hr, 8).shape) == (2, 1, 16, 16)    # = r (16 - 8): what the net returns


def test_clip_listing_and_shared_draws(pkg, tmp_path):
    """Items are three consecutive frames of ONE clip, frames sorted by name; one draw serves the three frames."""
    import contextlib
    import random
    from PIL import Image
    from pytorch_super_resolution_model_collection_amd import data
    rng = np.random.RandomState(0)
    for clip, n in (("b_clip", 5), ("a_clip", 3), ("short", 2)):
        os.makedirs(str(tmp_path / "vid" / clip))
        for i in reversed(range(n)):
            Image.fromarray(rng.randint(0, 256, (40, 48, 3), dtype=np.uint8)).save(str(tmp_path / "vid" / clip / ("f%03d.png" % i)))
    (tmp_path / "vid" / "stray.png").write_bytes(b"")          # a file beside the clip folders is not a clip
    ds = data.get_clip_training_set(str(tmp_path), ["vid"], 32, 2, is_gray=False, device="cpu")
    assert len(ds) == 1 + 3 + 0 and [os.path.basename(c) for c, _ in ds.clips] == ["a_clip", "b_clip", "short"]
    names = [tuple(os.path.relpath(f, str(tmp_path / "vid")) for f in it) for it in ds.items]
    assert names[0] == ("a_clip/f000.png", "a_clip/f001.png", "a_clip/f002.png")
    assert names[1:] == [tuple("b_clip/f%03d.png" % (i + k) for k in range(3)) for i in range(3)]
    assert ds.image_filenames == [it[1] for it in ds.items] and ds.decode_ahead is False
    assert ds.patcher.random_scale is False

    class FakeDev(object):
        device = "cpu"
        batch = staticmethod(contextlib.nullcontext)
        hand_over = staticmethod(lambda *t: t)
    seen = []

    def patch_u8(hwc, params, out=None):
        seen.append(params)
        out.copy_(torch.from_numpy(hwc[:32, :32].copy()).permute(2, 0, 1))
    ds.patcher._dev = FakeDev()
    ds.patcher.patch_u8 = patch_u8
    ds.patcher.finish = lambda patches: (patches[:, :, ::2, ::2].float(), patches.float(), None)
    random.seed(7)
    frames, hr = ds[2]
    state = random.getstate()
    assert len(seen) == 3 and seen[0] == seen[1] == seen[2] and seen[0][0] is None      # one draw, no random rescale
    assert tuple(frames.shape) == (3, 3, 16, 16) and tuple(hr.shape) == (3, 32, 32)
    want = torch.from_numpy(np.asarray(Image.open(str(tmp_path / "vid" / "b_clip" / "f002.png")))[:32, :32].copy())
    assert torch.equal(hr, want.permute(2, 0, 1).float())                               # the centre frame
    random.seed(7)
    ds[2]
    assert random.getstate() == state and seen[3] == seen[0]                            # the draws replay from `random`

    # the test walk: every frame of every clip once, with its neighbours, the ends using themselves
    ts = data.get_clip_test_set(str(tmp_path), "vid", 2, device="cpu")
    assert len(ts) == 3 + 5 + 2 and [ts.neighbours(i) for i in range(len(ts))] == (
        [(0, (0, 0, 1)), (0, (0, 1, 2)), (0, (1, 2, 2))]
        + [(1, (max(t - 1, 0), t, min(t + 1, 4))) for t in range(5)] + [(2, (0, 0, 1)), (2, (0, 1, 1))])
    loader = data.PatchLoader(ts, 1, shuffle=False, num_threads=1)
    assert loader._decode([0, 1]) == [(0, None), (1, None)]           # nothing is submitted to the decode pool


def test_video_window_schedule(pkg):
    """video_window / video_window_fill on frame numbers in place of frames, for both radii: every output sees (t-1, t, t+1)
    clamped to the stream (radius 1) or (t,) (radius 0), in order, as many outputs as frames, in the batches the
    restatement expects (radius 1) or in the reads as they come (radius 0)."""
    S = pkg.video_stream
    assert S.video_window(3, True, False, 1) == (5, 2, 2) and S.video_window(3, False, False, 1) == (5, 1, 3)
    assert S.video_window(1, False, True, 1) == (4, 1, 2) and S.video_window(0, False, True, 1) == (3, 1, 1)
    assert S.video_window(1, True, True, 1) == (4, 2, 1) and S.video_window(1, True, False, 1) == (3, 2, 0)
    assert S.video_window(3, True, False, 0) == (3, 0, 3) and S.video_window(0, False, True, 0) == (0, 0, 0)
    for R in (1, 0):
        for T in range(1, 14):
            for nb in range(1, 7):
                slots = [np.full(nb + 2 * R, -9), np.full(nb + 2 * R, -9)]
                seen, per_batch, reads, pos, b, kprev, first = [], [], [], 0, 0, 0, True
                while True:
                    k = min(nb, T - pos)
                    slots[b % 2][2 * R:2 * R + k] = np.arange(pos, pos + k)
                    reads.append((pos, pos + k))
                    pos += k
                    last = k < nb
                    before = slots[b % 2].copy()
                    S.video_window_fill(slots[b % 2], slots[(b - 1) % 2], k, kprev, first, last, R)
                    assert R or np.array_equal(slots[b % 2], before)          # radius 0 touches nothing
                    m, lo, n = S.video_window(k, first, last, R)
                    assert m <= nb + 2 * R and n <= nb
                    per_batch.append((len(seen), len(seen) + n))
                    seen += [tuple(int(v) for v in slots[b % 2][j - R:j + R + 1]) for j in range(lo, lo + n)]
                    kprev, first, b = k, False, b + 1
                    if last:
                        break
                if R:
                    assert seen == V.windows(T), (T, nb)
                    assert per_batch == V.output_batches(T, nb), (T, nb)
                else:
                    assert seen == [(t,) for t in range(T)], (T, nb)
                    assert per_batch == reads, (T, nb)
                    assert (T % nb == 0) == ((k, n) == (0, 0)), (T, nb)    # a multiple of the batch ends on an empty read
        with pytest.raises(ValueError, match="holds no frame"):
            S.video_window_fill(np.zeros(5), np.zeros(5), 0, 0, True, True, R)
