"""VESPCN's test_video on the device: frame t from frames (max(t-1, 0), t, min(t+1, T-1)), as many frames out as in, bytes
equal to tests/vespcn_ref.py's packing of the net's own fp32 output for the same batches, nothing allocated after the
first batch, at batch 3 and at batches where the first read yields nothing, the stream is an exact multiple and one short
read is all; the carries under a reader thread that waits for a pipe."""
import io
import os
import threading

import numpy as np
import pytest
import torch

import vespcn_ref as V
import video_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

STREAMS = {"420": "W24 H16 F25:1 Ip A1:1 C420jpeg", "mono": "W24 H16 F25:1 Cmono"}
_trainers = {}


def trainer(channels, gpu, tmp_path_factory):
    if channels not in _trainers:
        import main as cli
        from pytorch_super_resolution_model_collection_amd.sr_trainers import trainer_class
        args = cli.parse_args(["--model_name", "VESPCN", "--scale_factor", "2", "--num_channels", str(channels),
                               "--save_dir", str(tmp_path_factory.mktemp("vespcn%d" % channels))])
        t = trainer_class("VESPCN")(args)
        t.model = t.build_model()
        fill.fill_module(t.model, 5, 0.5)
        t.model.to(gpu).eval()
        _trainers[channels] = t
    return _trainers[channels]


def clip(kind, frames, seed=1):
    tokens = STREAMS[kind]
    sub = R.TAGS[[t for t in tokens.split() if t[0] == "C"][0]]
    rng = np.random.RandomState(seed)
    fb = R.layout(24, 16, sub)["frame_bytes"]
    ramp = (np.arange(fb) * 7 % 200 + 20).astype(np.int32)
    data = np.stack([np.clip(ramp + rng.randint(-20, 36, fb) + 9 * k, 0, 255) for k in range(frames)]).astype(np.uint8)
    return R.stream(tokens, data), tokens, sub, data


def check_restatement(t, gpu, kind, frames, channels, batch):
    data, tokens, sub, raw = clip(kind, frames)
    out = io.BytesIO()
    t.video_trace = seen = []
    try:
        assert t.test_video(io.BytesIO(data), out, batch=batch) == frames
    finally:
        t.video_trace = None
    with torch.no_grad():
        want, (OW, OH) = V.packed_video(lambda w: t.model(w), raw, 24, 16, sub, channels, batch, gpu)
    assert (OW, OH) == (2 * (24 - 8), 2 * (16 - 8))
    out_tokens = " ".join(("W%d" % OW) if k[0] == "W" else ("H%d" % OH) if k[0] == "H" else k for k in tokens.split())
    want = R.stream(out_tokens, want)
    got = out.getvalue()
    assert got[:got.index(b"\n") + 1] == want[:want.index(b"\n") + 1]
    assert len(R.parse(got)[4]) == frames and len(got) == len(want)       # as many frames as the input's
    diff = np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8)
    assert not diff.any(), "%d of %d bytes differ, first at %d" % (diff.sum(), diff.size, int(np.argmax(diff)))
    assert len(seen) == len(V.output_batches(frames, batch))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kind", ["420", "mono"])
@pytest.mark.parametrize("frames", [7, 6, 1])      # first, middle and short windows; the empty final read; one frame
def test_video_equals_the_restatement(gpu, tmp_path_factory, kind, frames, channels):
    check_restatement(trainer(channels, gpu, tmp_path_factory), gpu, kind, frames, channels, 3)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kind", ["420", "mono"])
@pytest.mark.parametrize("batch,frames", [(1, 3),      # the first batch yields no output; the flushing empty read
                                          (2, 4),      # an exact multiple
                                          (8, 4)])     # a single short read
def test_video_equals_the_restatement_at_other_batches(gpu, tmp_path_factory, kind, batch, frames, channels):
    check_restatement(trainer(channels, gpu, tmp_path_factory), gpu, kind, frames, channels, batch)


def test_video_from_a_slow_pipe_gives_the_same_bytes(gpu, tmp_path_factory):
    """Seven frames at batch 3 through an os.pipe in 777-byte pieces: the carries under a reader thread that waits for
    its source."""
    t = trainer(1, gpu, tmp_path_factory)
    data = clip("420", 7)[0]
    want = io.BytesIO()
    assert t.test_video(io.BytesIO(data), want, batch=3) == 7
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb") as f:
            for i in range(0, len(data), 777):
                f.write(data[i:i + 777])
                f.flush()
    th = threading.Thread(target=feed)
    th.start()
    sink = io.BytesIO()
    with os.fdopen(rd, "rb") as pipe:
        assert t.test_video(pipe, sink, batch=3) == 7
    th.join()
    assert sink.getvalue() == want.getvalue()


def test_video_allocates_nothing_after_the_first_batch(gpu, tmp_path_factory):
    t = trainer(1, gpu, tmp_path_factory)
    data = clip("420", 16)[0]
    t.video_trace = seen = []
    try:
        assert t.test_video(io.BytesIO(data), io.BytesIO(), batch=3) == 16
    finally:
        t.video_trace = None
    assert len(seen) == 6                      # five full reads and a short one
    print("memory_allocated at the end of each batch:", seen)
    assert len(set(seen[1:5])) == 1


def test_neighbours_matter_and_refusals(gpu, tmp_path_factory):
    """The output of a moving clip differs from the same frames run as their own neighbours; tile and self_ensemble are
    refused by name."""
    t = trainer(1, gpu, tmp_path_factory)
    data, _, sub, raw = clip("mono", 4)
    out = io.BytesIO()
    t.test_video(io.BytesIO(data), out, batch=3)
    got = R.parse(out.getvalue())[4]
    x = torch.from_numpy(R.unpack(raw, 24, 16, sub, 1)).to(gpu)
    with torch.no_grad():
        alone = t.model(x.unsqueeze(1).expand(-1, 3, -1, -1, -1).contiguous()).float().cpu().numpy()
    assert got.shape == R.pack(alone, sub).shape and not np.array_equal(got, R.pack(alone, sub))
    for kw in (dict(tile=16), dict(self_ensemble=True)):
        with pytest.raises(ValueError, match="without --tile and --self_ensemble"):
            t.test_video(io.BytesIO(data), io.BytesIO(), batch=3, **kw)
    with pytest.raises(ValueError, match="holds no frame"):
        t.test_video(io.BytesIO(R.stream(STREAMS["mono"], raw[:0])), io.BytesIO(), batch=3)
