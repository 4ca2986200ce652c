"""Integer numpy restatement of the JPEG round trip y = decode(encode(x, Q)) (include/srk.h): libjpeg's
baseline path without its lossless entropy coder -- the quality-scaled Annex-K tables, the integer colour tables, the 2x2
chroma shrink with its padding rules, the accurate integer DCT (jfdctint / jidctint), quantisation, the "fancy" triangle
upsampling and the colour tail.  Written from the definition, vectorised over whole planes; the C++ is not consulted.
Test infrastructure only; nothing here runs in the package.  CASES is the table the CPU and the GPU tests share."""
import random

import numpy as np

LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
        14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
          47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quant_table(quality, chroma):
    """The 8 x 8 table (natural order) of a quality clamped to 1..100."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array(CHROMA if chroma else LUMA, np.int64).reshape(8, 8)
    return np.clip((base * s + 50) // 100, 1, 255)


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's butterfly along the last axis; the first pass scales up by 2 bits, the second takes them back."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _idct_1d(c, n):
    """jidctint's butterfly along the last axis, results descaled by n bits."""
    c = [c[..., k] for k in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in out], axis=-1)


def _pad_to(p, mh, mw):
    """Replicate the last row / column of a plane out to multiples of (mh, mw)."""
    h, w = p.shape
    return np.pad(p, ((0, -h % mh), (0, -w % mw)), mode='edge')


def _codec(plane, table):
    """One padded plane (sides multiples of 8) through DCT, quantisation and back; int64 in, 0..255 out."""
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)          # [by, bx, row, col]
    c = _fdct_1d(b, True)                                                           # rows
    c = _fdct_1d(c.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)              # columns
    d = table << 3
    q = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    c = q * table
    s = _idct_1d(c.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)                 # columns first
    s = _idct_1d(s, 18)                                                             # then rows
    return np.clip(s + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _shrink(p):
    """The 2 x 2 chroma shrink of a full-size plane, padded as libjpeg pads it: columns of the source out to a multiple
    of 16, an odd height's last row once more, then the SHRUNK plane's last row down to a multiple of 8."""
    p = _pad_to(p, 2, 16)
    bias = np.array([1, 2] * (p.shape[1] // 4), np.int64)
    out = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad_to(out, 8, 8)


def _fancy(c, H, W):
    """The triangle filter over the ceil(H/2) x ceil(W/2) real samples of a decoded chroma plane, cropped to H x W.
    libjpeg takes it only for chroma planes wider than two samples; narrower ones (W <= 4) are replicated 2 x 2."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    c = c[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W]
    i, j = np.arange(ch), np.arange(cw)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    for v in (0, 1):
        s = 3 * c + c[np.clip(i - 1 if v == 0 else i + 1, 0, ch - 1)]
        out[v::2, 0::2] = (3 * s + s[:, np.clip(j - 1, 0, cw - 1)] + 8) >> 4
        out[v::2, 1::2] = (3 * s + s[:, np.clip(j + 1, 0, cw - 1)] + 7) >> 4
    return out[:H, :W]


def rgb_to_ycc(r, g, b):
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16)


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    return (np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255),
            np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255),
            np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255))


def jpeg_one(x, quality, subsampling=1, color=1):
    """One picture x uint8 [C, H, W] (C 1 or 3) -> uint8 [C, H, W].  quality 0: not compressed."""
    C, H, W = x.shape
    assert C in (1, 3) and not (color and C == 1) and subsampling in (0, 1)
    if int(quality) == 0:
        return x.copy()
    p = x.astype(np.int64)
    tl, tc = quant_table(quality, 0), quant_table(quality, 1)
    if C == 1:
        return _codec(_pad_to(p[0], 8, 8), tl)[:H, :W].astype(np.uint8)[None]
    y, cb, cr = rgb_to_ycc(p[0], p[1], p[2]) if color else (p[0], p[1], p[2])
    y = _codec(_pad_to(y, 8, 8), tl)[:H, :W]
    if subsampling:
        cb, cr = (_fancy(_codec(_shrink(c), tc), H, W) for c in (cb, cr))
    else:
        cb, cr = (_codec(_pad_to(c, 8, 8), tc)[:H, :W] for c in (cb, cr))
    out = ycc_to_rgb(y, cb, cr) if color else (y, cb, cr)
    return np.stack(out).astype(np.uint8)


def jpeg(x, quality, subsampling=1, color=1):
    """x uint8 [B, C, H, W]; quality an int, or one per patch."""
    q = [int(quality)] * x.shape[0] if np.ndim(quality) == 0 else [int(v) for v in quality]
    return np.stack([jpeg_one(x[b], q[b], subsampling, color) for b in range(x.shape[0])])


# -- Pillow's own round trip --------------------------------------------------------------------------------------------
def turbo():
    from PIL import features
    return bool(features.check_feature('libjpeg_turbo'))


def pillow_one(x, quality, subsampling=1, color=1):
    """Image.save(format='JPEG', quality=...) and Image.open of one picture [C, H, W]: mode L for C = 1, RGB for
    color = 1, else a YCbCr picture read back without libjpeg's colour tail (draft)."""
    import io
    from PIL import Image
    C = x.shape[0]
    buf = io.BytesIO()
    if C == 1:
        Image.fromarray(np.ascontiguousarray(x[0]), "L").save(buf, format="JPEG", quality=int(quality))
        return np.asarray(Image.open(io.BytesIO(buf.getvalue())), dtype=np.uint8)[None].copy()
    mode = "RGB" if color else "YCbCr"
    im = Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0)), mode)
    im.save(buf, format="JPEG", quality=int(quality), subsampling=2 if subsampling else 0)
    im = Image.open(io.BytesIO(buf.getvalue()))
    if not color:
        im.draft("YCbCr", None)
    im.load()
    assert im.mode == mode
    return np.ascontiguousarray(np.asarray(im, dtype=np.uint8).transpose(2, 0, 1))


# -- the case table -----------------------------------------------------------------------------------------------------
def content(kind, seed, shape):
    """Seeded 8-bit planes [C, H, W]: 'noise', 'smooth' (a ramp plus a little noise) or 'checker' (0 / 255 per pixel)."""
    rs = np.random.RandomState(seed)
    C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rs.randint(0, 256, shape).astype(np.uint8)
    if kind == "checker":
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), shape).copy()
    base = np.stack([110.0 + 70.0 * np.sin(xx / (3.0 + c) + seed) * np.cos(yy / (4.5 - c)) + 0.5 * (xx + yy) for c in range(C)])
    return np.clip(base + rs.normal(0, 6, shape), 0, 255).astype(np.uint8)


SIZES = [(1, 1), (7, 7), (8, 8), (16, 16), (17, 9), (23, 39), (32, 32), (33, 31), (34, 18), (40, 40), (70, 90)]
# (70 x 90 spans two of the kernel's 64 x 64 tiles in both directions, ragged; 34 x 18 and 40 x 40 are even with % 16 != 0:
#  the shrunk-row padding rule; 3 x 4 and 5 x 2 have a chroma plane of two samples or fewer: no triangle filter)
SMALL = [(3, 4), (5, 2)]


def _cases():
    """(name, kind, seed, (C, H, W), quality, subsampling, color).  Every size meets both contents, both subsamplings and
    the three picture kinds at rotating qualities; the 0/255 checkerboard, the hardest input for the clamp, rides on three
    sizes, the lowest quality (5) among them: the definition clamps where libjpeg's range-limit table would wrap, and
    tests/test_jpeg_cpu.py holds every case, these included, to Pillow's bytes -- no quality had to be raised."""
    rs = random.Random(24)
    quals = [5, 10, 30, 50, 75, 90, 95, 100]
    out, k = [], 0
    for (h, w) in SIZES + SMALL:
        for C, color in ((3, 1), (3, 0), (1, 0)):
            for sub in ((1, 0) if C == 3 else (0,)):
                kind = ("noise", "smooth")[k % 2]
                q = quals[k % len(quals)]
                out.append(("%s_%dx%d_c%d%s_s%d_q%d" % (kind, h, w, C, "rgb" if color else "", sub, q), kind,
                            rs.randrange(1 << 30), (C, h, w), q, sub, color))
                k += 1
    for (h, w), q in (((16, 16), 5), ((33, 31), 50), ((40, 40), 90)):
        out.append(("checker_%dx%d_q%d" % (h, w, q), "checker", 0, (3, h, w), q, 1, 1))
        out.append(("checker_%dx%d_grey_q%d" % (h, w, q), "checker", 0, (1, h, w), q, 0, 0))
    return out


CASES = _cases()
NAMES = [c[0] for c in CASES]


def case(name):
    for n, kind, seed, shape, q, sub, color in CASES:
        if n == name:
            return content(kind, seed, shape), q, sub, color
    raise KeyError(name)


BATCH_Q = [0, 1, 50, 100, 30]      # the batch case: one quality per patch, 0 = not compressed
BATCH_SHAPE = (5, 3, 32, 32)


def batch_case():
    x = np.stack([content(("noise", "smooth")[b % 2], 900 + b, BATCH_SHAPE[1:]) for b in range(BATCH_SHAPE[0])])
    return x, list(BATCH_Q)


# -- draws and the loader end to end (on top of degrade_ref's stages) -----------------------------------------------------
E2E_JPEG = dict(jpeg_quality=(30, 95), jpeg_prob=0.7)
TEST_JPEG = 40


def draw_jpeg(batch, jpeg_quality, jpeg_prob):
    """Consumes Python's `random` in the documented order: per patch random() < jpeg_prob, then randint(lo, hi)."""
    q = []
    for _ in range(batch):
        q.append(random.randint(*jpeg_quality) if random.random() < jpeg_prob else 0)
    return q


def noise_bytes(x, sigma, seed):
    import degrade_ref as R
    return np.clip(np.floor(R.noise_pre(x, sigma, seed)), 0.0, 255.0).astype(np.uint8)


def to_float(u8):
    return u8.astype(np.float32) / np.float32(255.0)


def replay_batches(folder, n_batches, is_gray=False, subsampling=1):
    """degrade_ref.replay_batches with the JPEG stage behind the noise: the first n_batches of an unshuffled PatchLoader
    over TrainDatasetFromFolder([folder], degrade=Degradation(**E2E['degradation'], **E2E_JPEG)) after random.seed(E2E
    ['seed']).  Per batch a dict with lr, hr, bc (fp32) and the qualities drawn."""
    import torch
    import degrade_ref as R
    from oracle import dataset_pil as O
    E = R.E2E
    ora = O.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=E['crop_size'], scale_factor=E['scale_factor'])
    d, B, lr_sz = E['degradation'], E['batch'], E['crop_size'] // E['scale_factor']
    random.seed(E['seed'])
    out = []
    for k in range(n_batches):
        hr = torch.stack([ora[i][1] for i in range(k * B, (k + 1) * B)]).numpy()
        patches = np.round(hr * np.float32(255.0)).astype(np.uint8)
        w, sigma, seed = R.draw(B, d['blur_prob'], d['blur_sigma'], d['noise_sigma'])
        q = draw_jpeg(B, **E2E_JPEG)
        u8 = noise_bytes(R.pil_resize(R.blur(patches, w), lr_sz, lr_sz), sigma, seed)
        lr = to_float(jpeg(u8, q, subsampling, 0 if is_gray else 1))
        out.append(dict(lr=lr, hr=hr, bc=R.bicubic_of_lr(lr, E['crop_size'], E['crop_size']), quality=q))
    return out


def item_lr_of_test_set(hwc, sf, degrade, index, quality, is_gray=False, subsampling=1):
    """TestDatasetFromFolder's lr of a decoded image [H, W, C] under jpeg=quality, behind the fixed degradation `degrade`
    (or None: the clean shrink)."""
    import degrade_ref as R
    h, w, c = hwc.shape
    lr_h, lr_w = (h - h % sf) // sf, (w - w % sf) // sf
    planes = np.ascontiguousarray(hwc.transpose(2, 0, 1))[None]
    if degrade is not None:
        s1, s2, th, ns = degrade
        planes = R.blur(planes, R.blur_weights(s1, s2, th, R.kernel_size(s1, s2))[None])
    u8 = R.pil_resize(planes, lr_h, lr_w)
    if degrade is not None:
        u8 = noise_bytes(u8, [degrade[3]], index)
    return to_float(jpeg(u8, quality, subsampling, 0 if is_gray else 1))[0]
