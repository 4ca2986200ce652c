"""The video path without a GPU: the YUV4MPEG2 container (data.Y4MReader / Y4MWriter), the one layout function
(ops.yuv_layout), and the host twins of the two kernels (srk_yuv_unpack_host / srk_yuv_pack_host, which compile the
kernels' per-pixel header) against the numpy / Pillow restatement of tests/video_ref.py: every byte and every fp32 value
equal, nothing left out.  The device kernels are held to the host twins on the same table in tests/test_video_gpu.py."""
import ctypes
import io
import os
import threading

import numpy as np
import pytest
from PIL import Image

import __graft_entry__
import video_ref as R


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def read_all(pkg, src, batch):
    """(header, frames [N, frame_bytes], batch sizes) through Y4MReader.batches over two rotating buffers."""
    with pkg.data.Y4MReader(src) as r:
        bufs = [np.zeros((batch, r.layout.frame_bytes), np.uint8) for _ in range(2)]
        got, sizes = [], []
        for buf, k in r.batches(bufs, batch):
            got.append(buf[:k].copy())
            sizes.append(k)
        return r.header, (np.concatenate(got) if got else np.zeros((0, r.layout.frame_bytes), np.uint8)), sizes


# ---- the layout function ----

@pytest.mark.parametrize("W,H,sub", R.SIZES)
def test_layout_function(pkg, W, H, sub):
    lay, want = pkg.ops.yuv_layout(W, H, sub), R.layout(W, H, sub)
    assert (lay.W, lay.H, lay.sub) == (W, H, sub)
    for key, val in want.items():
        assert getattr(lay, key) == val, key
    assert lay.scaled(2 * W, 2 * H).frame_bytes == 4 * lay.frame_bytes
    assert lay.code == {"420": 0, "444": 1, "mono": 2}[sub]


def test_layout_numbers_and_refusals(pkg):
    lay = pkg.ops.yuv_layout(6, 4, "420")
    assert (lay.frame_bytes, lay.cb_off, lay.cr_off, lay.cw, lay.ch) == (36, 24, 30, 3, 2)   # frame 1 starts at byte 36
    assert pkg.ops.yuv_layout(7, 5, "444").frame_bytes == 105 and pkg.ops.yuv_layout(5, 3, "mono").frame_bytes == 15
    for w, h in ((7, 4), (6, 5)):
        with pytest.raises(ValueError, match="C420mpeg2.*W%d H%d" % (w, h)):
            pkg.ops.yuv_layout(w, h, "420", "C420mpeg2")
    with pytest.raises(ValueError, match="422"):
        pkg.ops.yuv_layout(6, 4, "422")
    with pytest.raises(ValueError):
        pkg.ops.yuv_layout(0, 4, "444")


# ---- the container ----

@pytest.mark.parametrize("tag", sorted(R.TAGS) + [None])
def test_container_accepts_and_round_trips(pkg, tag):
    sub = R.TAGS[tag or "C420jpeg"]
    W, H = (6, 4) if sub == "420" else (7, 5)
    tokens = "W%d H%d F30000:1001 Ip A1:1%s XYSCSS=%s XCOLORRANGE=FULL" % (W, H, " " + tag if tag else "", sub.upper())
    frames = R.random_frames(11, 5, W, H, sub)
    data = R.stream(tokens, frames)
    head, got, sizes = read_all(pkg, io.BytesIO(data), 2)
    assert sizes == [2, 2, 1] and np.array_equal(got, frames)
    assert (head.W, head.H, head.chroma_tag, head.layout.sub) == (W, H, tag, sub)
    assert head.layout == pkg.ops.yuv_layout(W, H, sub)
    sink = io.BytesIO()
    w = pkg.data.Y4MWriter(sink, head)
    w.write(got[:3])
    w.write(got[3:], 2)
    w.close()
    assert sink.getvalue() == data and w.frames_written == 5
    # FRAME lines with parameters are read, and written back bare
    noisy = R.stream(tokens, frames, b"FRAME Ip XNOTE=1\n")
    head2, got2, _ = read_all(pkg, io.BytesIO(noisy), 8)
    assert np.array_equal(got2, frames) and head2.line() == head.line()
    # the output side's header: W and H replaced, everything else carried through in place
    up = head.scaled(3 * W, 2 * H)
    assert up.line() == ("YUV4MPEG2 " + tokens.replace("W%d" % W, "W%d" % (3 * W)).replace("H%d" % H, "H%d" % (2 * H)) + "\n").encode()
    assert up.layout == pkg.ops.yuv_layout(3 * W, 2 * H, sub)


def test_container_header_without_optional_tags(pkg):
    head, got, _ = read_all(pkg, io.BytesIO(R.stream("W2 H2", R.random_frames(1, 1, 2, 2, "420"))), 4)
    assert head.layout.sub == "420" and got.shape == (1, 6) and head.line() == b"YUV4MPEG2 W2 H2\n"
    assert read_all(pkg, io.BytesIO(R.stream("W2 H2 I?", np.zeros((0, 6), np.uint8))), 4)[1].shape == (0, 6)


@pytest.mark.parametrize("tokens,names", [("W6 H4 C422", "C422"), ("W6 H4 C420p10", "C420p10"), ("W6 H4 C444alpha", "C444alpha"),
                                          ("W6 H4 C444p16", "C444p16"), ("W6 H4 It", "It"), ("W6 H4 Ib C420jpeg", "Ib"),
                                          ("W6 H4 Im", "Im"), ("W7 H4 C420jpeg", "C420jpeg.*W7 H4"), ("W6 H5", "C420jpeg.*W6 H5"),
                                          ("W6 H4 Q1", "Q1"), ("H4 C444", "no W tag"), ("W6 Hx", "Hx")])
def test_container_refusals_name_the_tag(pkg, tokens, names):
    with pytest.raises(ValueError, match=names):
        pkg.data.Y4MReader(io.BytesIO(R.stream(tokens, np.zeros((1, 36), np.uint8))))


def test_container_refuses_other_streams_and_truncation(pkg):
    with pytest.raises(ValueError, match="not a YUV4MPEG2 stream"):
        pkg.data.Y4MReader(io.BytesIO(b"RIFF....AVI LIST\n"))
    frames = R.random_frames(3, 3, 6, 4, "420")
    data = R.stream("W6 H4 C420jpeg", frames)
    with pytest.raises(ValueError, match="frame 2 ends early: got 29 bytes, expected 36"):
        read_all(pkg, io.BytesIO(data[:-7]), 2)
    with pytest.raises(ValueError, match="frame 1 does not begin with a FRAME line"):
        read_all(pkg, io.BytesIO(data.replace(b"FRAME\n", b"FRAMX\n").replace(b"FRAMX\n", b"FRAME\n", 1)), 2)
    with pytest.raises(ValueError, match="holds no frame"):
        pkg.data.Y4MReader(io.BytesIO(data)).read_into(np.zeros(35, np.uint8))


def test_container_sources_path_bytesio_and_pipe(pkg, tmp_path):
    import torch
    frames = R.random_frames(5, 7, 34, 22, "420")
    data = R.stream("W34 H22 F25:1 C420mpeg2", frames)
    path = tmp_path / "in.y4m"
    path.write_bytes(data)
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb") as f:
            for i in range(0, len(data), 1000):   # pieces that end inside frames and inside FRAME lines
                f.write(data[i:i + 1000])
                f.flush()
    th = threading.Thread(target=feed)
    th.start()
    with os.fdopen(rd, "rb") as pipe:
        from_pipe = read_all(pkg, pipe, 3)
    th.join()
    for head, got, sizes in (read_all(pkg, str(path), 3), read_all(pkg, io.BytesIO(data), 3), from_pipe):
        assert sizes == [3, 3, 1] and np.array_equal(got, frames) and head.chroma_tag == "C420mpeg2"
    # a torch buffer is filled in place: dense payloads, frame 1 at byte frame_bytes
    buf = torch.zeros((4, 34 * 22 * 3 // 2), dtype=torch.uint8)
    with pkg.data.Y4MReader(str(path)) as r:
        assert r.read_into(buf, 4) == 4 and r.read_into(buf[:2]) == 2 and r.read_into(buf) == 1 and r.read_into(buf) == 0
        assert r.frames_read == 7
    assert np.array_equal(buf.numpy()[:1], frames[6:7]) and np.array_equal(buf.numpy()[2:], frames[2:4])
    out = tmp_path / "deep" / "dir" / "out.y4m"
    with pkg.data.Y4MWriter(str(out), pkg.data.Y4MReader(io.BytesIO(data)).header) as w:
        w.write(frames)
    assert out.read_bytes() == data


# ---- the host twins against the restatement ----

def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                         b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("n", R.BATCHES)
@pytest.mark.parametrize("W,H,sub", R.SIZES)
def test_unpack_host_twin_equals_the_restatement(pkg, W, H, sub, n, channels):
    frames = R.random_frames(W * 100 + H + n, n, W, H, sub)
    lay = pkg.ops.yuv_layout(W, H, sub)
    full = R.chroma_planes(frames, W, H, sub, W, H) if (sub == "420" and channels == 3) else None
    got = pkg.ops.yuv_unpack_host(frames, lay, channels, full)
    assert same_bits(got, R.unpack(frames, W, H, sub, channels))
    # a frame stride beyond the payload, and a first byte off every alignment
    wide = np.zeros((n, lay.frame_bytes + 5), np.uint8)
    wide[:, :lay.frame_bytes] = frames
    assert same_bits(pkg.ops.yuv_unpack_host(wide, lay, channels, full), got)
    flat = np.zeros(n * lay.frame_bytes + 1, np.uint8)
    flat[1:] = frames.reshape(-1)
    assert same_bits(pkg.ops.yuv_unpack_host(flat[1:].reshape(n, lay.frame_bytes), lay, channels, full), got)


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("n", R.BATCHES)
@pytest.mark.parametrize("W,H,sub", R.SIZES)
def test_pack_host_twin_equals_the_restatement(pkg, W, H, sub, n, channels):
    y = R.net_output(W * 7 + H + n + channels, n, channels, H, W)
    lay = pkg.ops.yuv_layout(W, H, sub)
    chroma = None
    if channels == 1 and sub != "mono":
        chroma = np.random.RandomState(W + H).randint(0, 256, (2, n, lay.ch, lay.cw)).astype(np.uint8)
    want = R.pack(y, sub, chroma)
    got = pkg.ops.yuv_pack_host(y, lay, chroma)
    assert got.shape == (n, lay.frame_bytes) and np.array_equal(got, want)
    last = np.ascontiguousarray(y.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)   # a channels-last output, read in place
    assert np.array_equal(pkg.ops.yuv_pack_host(last, lay, chroma), want)
    big = np.full((n, channels, H + 3, W + 5), np.float32(0.5))
    big[:, :, 1:H + 1, 2:W + 2] = y
    assert np.array_equal(pkg.ops.yuv_pack_host(big[:, :, 1:H + 1, 2:W + 2], lay, chroma), want)


def test_quantisation_branches_by_value(pkg):
    """The pack inputs of the table reach every branch, and the named values quantise as the definition says, in the
    restatement and in the host twin alike."""
    v = R.net_output(3, 1, 3, 22, 34)
    assert np.isnan(v).any() and (v < 0).any() and (v > 1).any() and np.isinf(v).any()
    k = v[np.isfinite(v)] * np.float32(255.0)
    assert ((k == np.round(k)) & (k > 0) & (k < 255)).sum() > 100      # exact multiples of 1 / 255
    named = np.array([np.nan, -1, 0, 0.5, 1, 2, np.inf, -np.inf, 254.999 / 255, 1 / 255, -0.0, 1e-9], np.float32)
    want = [0, 0, 0, 127, 255, 255, 255, 0, 254, 1, 0, 0]
    assert R.quantise(named).tolist() == want
    got = pkg.ops.yuv_pack_host(named.reshape(1, 1, 3, 4), pkg.ops.yuv_layout(4, 3, "mono"))
    assert got.reshape(-1).tolist() == want
    levels = (np.arange(256, dtype=np.float32) / np.float32(255.0)).reshape(1, 1, 16, 16)      # ToTensor's values come back
    assert pkg.ops.yuv_pack_host(levels, pkg.ops.yuv_layout(16, 16, "mono")).reshape(-1).tolist() == list(range(256))


def test_dash_means_the_binary_standard_streams(pkg, monkeypatch):
    """'-' as a source is stdin's byte stream, as a sink stdout's; neither is closed."""
    import sys

    class Std(object):
        def __init__(self, data=b""):
            self.buffer = io.BytesIO(data)
    frames = R.random_frames(2, 3, 6, 4, "420")
    data = R.stream("W6 H4 F25:1 C420jpeg", frames)
    stdin, stdout = Std(data), Std()
    monkeypatch.setattr(sys, "stdin", stdin)
    monkeypatch.setattr(sys, "stdout", stdout)
    head, got, sizes = read_all(pkg, "-", 2)
    with pkg.data.Y4MWriter("-", head) as w:
        w.write(got)
    monkeypatch.undo()
    assert sizes == [2, 1] and np.array_equal(got, frames)
    assert stdout.buffer.getvalue() == data and not stdout.buffer.closed and not stdin.buffer.closed


def test_chroma_shrink_is_pillows_box_not_the_mean(pkg):
    """The fused 2 x 2 shrink of the RGB tail, held to Image.resize(..., Image.BOX) directly; and the closed form of the
    restatement on all 65536 sample pairs."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    pairs = np.stack([a.reshape(-1), b.reshape(-1)], 1).reshape(1, -1).astype(np.uint8)      # a0 b0 a1 b1 ...
    assert np.array_equal(R.box_half(np.concatenate([pairs, pairs])), R.box_closed_form(np.concatenate([pairs, pairs])))
    cols = np.concatenate([pairs[:, 0::2], pairs[:, 1::2]])                                  # column pairs
    assert np.array_equal(R.box_half(np.repeat(cols, 2, axis=1)), R.box_closed_form(np.repeat(cols, 2, axis=1)))
    differs = 0
    for seed, (W, H) in enumerate([(34, 22), (64, 48), (6, 4), (2, 2)]):
        rgb = np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
        y = (rgb.transpose(2, 0, 1)[None].astype(np.float32) / np.float32(255.0))
        assert np.array_equal(R.quantise(y)[0].transpose(1, 2, 0), rgb)
        lay = pkg.ops.yuv_layout(W, H, "420")
        frame = pkg.ops.yuv_pack_host(y, lay)[0]
        yy, cb, cr = Image.fromarray(rgb).convert("YCbCr").split()
        assert np.array_equal(frame[:W * H].reshape(H, W), np.asarray(yy))
        for plane, off in ((cb, lay.cb_off), (cr, lay.cr_off)):
            want = np.asarray(plane.resize((W // 2, H // 2), Image.BOX))
            assert np.array_equal(frame[off:off + lay.cw * lay.ch].reshape(lay.ch, lay.cw), want)
            p = np.asarray(plane).astype(np.int32)
            mean = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
            differs += int((mean != want).sum())
    assert differs > 0      # the four-sample mean is a different function


def test_rgb_conversions_are_pillows(pkg):
    """Both directions on 4:4:4 frames, against Image.merge('YCbCr', ...).convert('RGB') and back."""
    W, H = 64, 48
    frames = R.random_frames(21, 2, W, H, "444")
    lay = pkg.ops.yuv_layout(W, H, "444")
    x = pkg.ops.yuv_unpack_host(frames, lay, 3)
    for n in range(2):
        ycc = frames[n].reshape(3, H, W)
        rgb = np.asarray(Image.merge("YCbCr", [Image.fromarray(p) for p in ycc]).convert("RGB"))
        assert same_bits(x[n], rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))
        back = np.stack([np.asarray(p) for p in Image.fromarray(rgb).convert("YCbCr").split()])
        assert np.array_equal(pkg.ops.yuv_pack_host(x[n:n + 1], lay)[0].reshape(3, H, W), back)
    mono = pkg.ops.yuv_unpack_host(frames[:, :W * H], pkg.ops.yuv_layout(W, H, "mono"), 3)
    grey = np.asarray(Image.merge("YCbCr", [Image.fromarray(frames[0, :W * H].reshape(H, W))]
                                  + [Image.new("L", (W, H), 128)] * 2).convert("RGB"))
    assert same_bits(mono[0], grey.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))


def test_unpack_then_pack_of_a_y_model_is_the_identity(pkg):
    for W, H, sub in R.SIZES:
        frames = R.random_frames(9, 2, W, H, sub)
        lay = pkg.ops.yuv_layout(W, H, sub)
        chroma = None if sub == "mono" else np.stack([np.stack([R.planes(f, W, H, sub)[k] for f in frames]) for k in (1, 2)])
        assert np.array_equal(pkg.ops.yuv_pack_host(pkg.ops.yuv_unpack_host(frames, lay, 1), lay, chroma), frames)


# ---- error returns ----

def test_entry_points_return_errors(pkg, lib):
    frames = np.zeros((2, 36), np.uint8)
    full = np.zeros((2, 2, 4, 6), np.uint8)
    x1, x3 = np.zeros((2, 1, 4, 6), np.float32), np.zeros((2, 3, 4, 6), np.float32)
    chroma = np.zeros((2, 2, 2, 3), np.uint8)
    out = np.zeros((2, 3, 4, 6), np.float32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    st = lambda a: (ctypes.c_int64 * 4)(*[s // 4 for s in a.strides])

    def unpack(fn, extra, frames=frames, stride=36, n=2, h=4, w=6, sub=0, c=3, full=full, out=out):
        return fn(p(frames), stride, n, h, w, sub, c, p(full), p(out), *extra)

    def pack(fn, extra, x=x3, strides=None, n=2, c=3, h=4, w=6, sub=0, chroma=None, frames=frames, stride=36):
        return fn(p(x), st(x) if strides is None else strides, n, c, h, w, sub, p(chroma), p(frames), stride, *extra)

    for fn, extra in ((lib.srk_yuv_unpack_host, ()), (lib.srk_yuv_unpack, (None,))):
        for kw, match in ((dict(frames=None), b"null pointer"), (dict(out=None), b"null pointer"),
                          (dict(n=0), b"non-positive sizes (N = 0"), (dict(h=0), b"non-positive sizes"),
                          (dict(w=-6), b"non-positive sizes"), (dict(c=2), b"C must be 1 or 3 (got 2)"),
                          (dict(sub=3), b"unknown subsampling code 3"), (dict(h=5), b"odd size (6 x 5)"),
                          (dict(w=7), b"odd size (7 x 4)"), (dict(stride=35), b"frame stride 35 < the frame's 36 bytes"),
                          (dict(full=None), b"needs the full-resolution chroma planes")):
            assert unpack(fn, extra, **kw) == -1, kw
            assert match in lib.srk_last_error_string(), (kw, lib.srk_last_error_string())
    assert unpack(lib.srk_yuv_unpack_host, (), full=None, c=1, out=np.zeros((2, 1, 4, 6), np.float32)) == 0   # not needed there
    neg = (ctypes.c_int64 * 4)(72, 24, -6, 1)
    for fn, extra in ((lib.srk_yuv_pack_host, ()), (lib.srk_yuv_pack, (None,))):
        for kw, match in ((dict(x=None, strides=st(x3)), b"null pointer"), (dict(frames=None), b"null pointer"),
                          (dict(n=0), b"non-positive sizes"), (dict(c=4), b"C must be 1 or 3 (got 4)"),
                          (dict(sub=-1), b"unknown subsampling code -1"), (dict(h=3), b"odd size (6 x 3)"),
                          (dict(stride=10), b"frame stride 10 < the frame's 36 bytes"), (dict(strides=neg), b"negative strides"),
                          (dict(x=x1, c=1), b"needs the resized chroma planes")):
            assert pack(fn, extra, **kw) == -1, kw
            assert match in lib.srk_last_error_string(), (kw, lib.srk_last_error_string())
    assert pack(lib.srk_yuv_pack_host, (), x=x1, c=1, chroma=chroma) == 0
    with pytest.raises(RuntimeError, match="needs the resized chroma planes"):
        pkg.ops.yuv_pack_host(x1, pkg.ops.yuv_layout(6, 4, "420"))
    with pytest.raises(ValueError, match="chroma must be"):
        pkg.ops.yuv_pack_host(x1, pkg.ops.yuv_layout(6, 4, "420"), chroma[:, :1])
    with pytest.raises(ValueError, match="float32"):
        pkg.ops.yuv_pack_host(x1.astype(np.float64), pkg.ops.yuv_layout(6, 4, "420"), chroma)


# ---- the surface ----

def test_cli_carries_the_video_flags(tmp_path, capsys):
    import main as cli
    base = ["--save_dir", str(tmp_path)]
    plain = cli.parse_args(base)
    assert plain.test_video is None and plain.video_out is None and plain.video_batch == 8
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(R.stream("W2 H2", R.random_frames(0, 1, 2, 2, "420")))
    a = cli.parse_args(base + ["--test_video", str(clip), "--video_out", "-", "--video_batch", "3", "--tile", "16"])
    assert (a.test_video, a.video_out, a.video_batch, a.tile) == (str(clip), "-", 3, 16)
    keys = ("test_video", "video_out", "video_batch", "tile")
    assert {k: v for k, v in vars(a).items() if k not in keys} == {k: v for k, v in vars(plain).items() if k not in keys}
    assert cli.parse_args(base + ["--test_video", "-"]).test_video == "-"
    for argv, match in ((["--test_video", str(tmp_path / "none.y4m")], "none.y4m: no such file"),
                        (["--video_out", "x.y4m"], "goes with --test_video"),
                        (["--test_video", str(clip), "--video_batch", "0"], "must be positive"),
                        (["--test_video", str(clip), "--test_only"], "does not go with --test_only"),
                        (["--test_video", str(clip), "--test_single", "x.png"], "does not go with --test_single")):
        with pytest.raises(SystemExit):
            cli.parse_args(base + argv)
        assert match in capsys.readouterr().err, argv


def test_header_integration_and_build_name_the_new_unit(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for sym in ("srk_yuv_unpack", "srk_yuv_pack", "srk_yuv_unpack_host", "srk_yuv_pack_host"):
        assert sym in pkg._lib.header_symbols() and sym in pkg._lib._PROTOTYPES
        assert sym in open(os.path.join(root, "INTEGRATION.md")).read(), sym
    assert "video.hip" in pkg._build.SOURCES and "video_common.h" in pkg._build.HEADERS
    from pytorch_super_resolution_model_collection_amd import sr_trainers
    assert hasattr(sr_trainers._Trainer, "test_video")
