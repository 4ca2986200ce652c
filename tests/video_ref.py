"""The yardstick of the video path: a numpy / Pillow restatement of the YUV4MPEG2 container, the frame layout, the front
(frame bytes -> the net's fp32 input) and the tail (the net's fp32 output -> frame bytes), written from the definition and
not from the kernels.

Definition.  A stream is "YUV4MPEG2 W.. H.. [tags]\\n", then per frame "FRAME[ params]\\n" and the payload: the 8-bit Y
plane [H][W], then for 4:2:0 Cb and Cr [ceil(H/2)][ceil(W/2)], for 4:4:4 Cb and Cr [H][W], for mono nothing.  Samples are
full-range JFIF values.
  front, Y model:   Y / 255 in fp32 (ToTensor).
  front, RGB model: Image.merge('YCbCr', (Y, Cb, Cr)).convert('RGB'), / 255, planar; Cb / Cr at full size are the frame's
                    own (4:4:4), Pillow's bicubic resize of the frame's (4:2:0), or the constant 128 (mono).
  tail:             every value v becomes (uint8)(clamp(v, 0, 1) * 255) with the fp32 product truncated, NaN -> 0
                    (ToPILImage after clamp).  Y model: that plane, with Cb / Cr planes handed in (the pipeline makes them
                    with Pillow's bicubic resize of the input's chroma to the output's chroma size).  RGB model:
                    Image.convert('YCbCr') of the quantised picture; 4:4:4 keeps Cb / Cr, 4:2:0 takes
                    resize((OW / 2, OH / 2), Image.BOX) of each, mono drops them."""
import numpy as np
from PIL import Image

# the table of the CPU and GPU kernel tests: (W, H, subsampling)
SIZES = [(2, 2, "420"), (6, 4, "420"), (34, 22, "420"), (64, 48, "420"), (7, 5, "444"), (5, 3, "mono")]
BATCHES = (1, 3)
TAGS = {"C420jpeg": "420", "C420mpeg2": "420", "C420paldv": "420", "C420": "420", "C444": "444", "Cmono": "mono"}


def layout(W, H, sub):
    """dict(cw, ch, y_off, cb_off, cr_off, frame_bytes) of one frame."""
    if sub == "420":
        cw, ch = -(-W // 2), -(-H // 2)
    elif sub == "444":
        cw, ch = W, H
    else:
        cw, ch = 0, 0
    return dict(cw=cw, ch=ch, y_off=0, cb_off=W * H, cr_off=W * H + cw * ch, frame_bytes=W * H + 2 * cw * ch)


def planes(frame, W, H, sub):
    """(y, cb, cr) views of one frame's bytes; cb = cr = None for mono."""
    L = layout(W, H, sub)
    y = frame[:W * H].reshape(H, W)
    if sub == "mono":
        return y, None, None
    n = L["cw"] * L["ch"]
    return y, frame[L["cb_off"]:L["cb_off"] + n].reshape(L["ch"], L["cw"]), frame[L["cr_off"]:L["cr_off"] + n].reshape(L["ch"], L["cw"])


def random_frames(seed, n, W, H, sub):
    return np.random.RandomState(seed).randint(0, 256, (n, layout(W, H, sub)["frame_bytes"])).astype(np.uint8)


def bicubic(plane, ow, oh):
    return np.asarray(Image.fromarray(np.ascontiguousarray(plane)).resize((ow, oh), Image.BICUBIC))


def chroma_planes(frames, W, H, sub, ow, oh):
    """[2, N, oh, ow]: Pillow's bicubic resize of every frame's Cb and Cr planes."""
    out = np.empty((2, len(frames), oh, ow), np.uint8)
    for n, f in enumerate(frames):
        _, cb, cr = planes(f, W, H, sub)
        out[0, n], out[1, n] = bicubic(cb, ow, oh), bicubic(cr, ow, oh)
    return out


def unpack(frames, W, H, sub, channels):
    """[N, frame_bytes] uint8 -> float32 [N, channels, H, W]."""
    out = np.empty((len(frames), channels, H, W), np.float32)
    for n, f in enumerate(frames):
        y, cb, cr = planes(f, W, H, sub)
        if channels == 1:
            out[n, 0] = y.astype(np.float32) / np.float32(255.0)
            continue
        if sub == "mono":
            cb = cr = np.full((H, W), 128, np.uint8)
        elif sub == "420":
            cb, cr = bicubic(cb, W, H), bicubic(cr, W, H)
        img = Image.merge("YCbCr", [Image.fromarray(np.ascontiguousarray(p)) for p in (y, cb, cr)]).convert("RGB")
        out[n] = np.asarray(img).transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return out


def quantise(v):
    v = np.asarray(v, np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return (np.clip(v, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8)


def box_half(plane):
    h, w = plane.shape
    return np.asarray(Image.fromarray(np.ascontiguousarray(plane)).resize((w // 2, h // 2), Image.BOX))


def box_closed_form(plane):
    """The closed form of box_half: rounded after the row pass and again after the column pass."""
    p = plane.astype(np.int32)
    h = (p[:, 0::2] + p[:, 1::2] + 1) >> 1
    return ((h[0::2] + h[1::2] + 1) >> 1).astype(np.uint8)


def pack(y, sub, chroma=None):
    """float32 [N, C, OH, OW] -> [N, frame_bytes] uint8 of OW x OH frames.  chroma: [2, N, ch, cw] for C = 1 (not mono)."""
    y = np.asarray(y)
    N, C, OH, OW = y.shape
    L = layout(OW, OH, sub)
    out = np.zeros((N, L["frame_bytes"]), np.uint8)
    q = quantise(y)
    for n in range(N):
        if C == 1:
            parts = [q[n, 0]] + ([] if sub == "mono" else [chroma[0, n], chroma[1, n]])
        else:
            yy, cb, cr = (np.asarray(p) for p in Image.fromarray(np.ascontiguousarray(q[n].transpose(1, 2, 0))).convert("YCbCr").split())
            parts = [yy] if sub == "mono" else [yy, cb, cr] if sub == "444" else [yy, box_half(cb), box_half(cr)]
        out[n] = np.concatenate([np.asarray(p).reshape(-1) for p in parts])
    return out


def net_output(seed, n, c, oh, ow):
    """A stand-in for a net's output that reaches every branch of the quantisation: values below 0 and above 1, exact
    multiples of 1 / 255, 0 and 1 themselves, NaN and both infinities."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(-0.25, 1.25, (n, c, oh, ow)).astype(np.float32)
    flat = v.reshape(-1)
    k = rng.randint(0, 256, flat.size).astype(np.float32) / np.float32(255.0)
    flat[0::3] = k[0::3]
    special = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0, 1.0 / 255, 254.5 / 255], np.float32)
    idx = rng.permutation(flat.size)[:min(flat.size, 2 * special.size)]
    flat[idx] = np.resize(special, idx.size)
    return v


def stream(tokens, frames, frame_line=b"FRAME\n"):
    """The bytes of a stream: tokens is the header after the magic ('W6 H4 F25:1 ...'), frames [N, frame_bytes]."""
    out = [b"YUV4MPEG2 " + tokens.encode() + b"\n"]
    for f in frames:
        out += [frame_line, np.ascontiguousarray(f).tobytes()]
    return b"".join(out)


def parse(data):
    """(header tokens as one string, W, H, sub, frames [N, frame_bytes]) of a stream's bytes; FRAME parameters are dropped."""
    end = data.index(b"\n")
    head = data[:end].decode().split(" ")
    assert head[0] == "YUV4MPEG2"
    W = int([t for t in head if t.startswith("W")][0][1:])
    H = int([t for t in head if t.startswith("H")][0][1:])
    ctag = ([t for t in head if t.startswith("C")] or ["C420jpeg"])[0]
    sub = TAGS[ctag]
    fb = layout(W, H, sub)["frame_bytes"]
    frames, pos = [], end + 1
    while pos < len(data):
        e = data.index(b"\n", pos)
        assert data[pos:pos + 5] == b"FRAME"
        frames.append(np.frombuffer(data[e + 1:e + 1 + fb], np.uint8))
        assert len(frames[-1]) == fb
        pos = e + 1 + fb
    return " ".join(head[1:]), W, H, sub, np.stack(frames) if frames else np.zeros((0, fb), np.uint8)
