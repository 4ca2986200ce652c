"""numpy / Pillow / scipy restatement of Real-ESRGAN's second-order degradation on 8-bit stage boundaries (include/srk.h,
DESIGN.md 32): the four kinds of blur table, the Poisson inversion table, the Gaussian / Poisson / gray noise, the unsharp
mask, the draws of data.Degradation2 from a `random` generator and the whole chain with Pillow's Image.resize in the middle
and jpeg_ref's libjpeg restatement for the JPEG stages.  Every operator also returns the fp64 values about to be rounded or
compared, so that the CPU suite can assert that none lies within 1e-7 of a boundary.  Test infrastructure
only; nothing here runs in the package."""
import math
import random

import numpy as np

import degrade_ref as R1
import jpeg_ref as J

KT, PEAK = 448, 256.0
OFF, GAUSS, POISSON = 0, 1, 2
BOX, BILINEAR, BICUBIC = 4, 2, 3
FILTERS = (BOX, BILINEAR, BICUBIC)
KINDS = (("gauss", False), ("gauss", True), ("ggauss", False), ("ggauss", True), ("plateau", False), ("plateau", True))
GUARD = 1e-7


# -- blur tables ------------------------------------------------------------------------------------------------------
def _j1(x):
    from scipy.special import j1
    return float(j1(x))


def blur_table(kind, K, s1=1.0, s2=1.0, theta=0.0, beta=1.0, cutoff=1.0):
    """The normalised K x K table, row-major; scalar fp64 arithmetic in the documented order, the sum by math.fsum."""
    r = K // 2
    c, s = math.cos(theta), math.sin(theta)
    w = np.zeros((K, K), np.float64)
    for i in range(K):
        for j in range(K):
            x, y = float(j - r), float(i - r)
            if kind == "sinc":
                rr = math.sqrt(x * x + y * y)
                w[i, j] = cutoff * cutoff / (4.0 * math.pi) if rr == 0.0 else cutoff * _j1(cutoff * rr) / (2.0 * math.pi * rr)
                continue
            u, v = c * x + s * y, -s * x + c * y
            q = u * u / (s1 * s1) + v * v / (s2 * s2)
            w[i, j] = (math.exp(-0.5 * q) if kind == "gauss" else math.exp(-0.5 * q ** beta) if kind == "ggauss"
                       else 1.0 / (1.0 + q ** beta))
    return _normalised(w)


def _normalised(w):
    """w / sum(w), the centre entry then taking up what the rounded entries' sum lacks from 1."""
    w = w / math.fsum(w.ravel())
    flat = w.reshape(-1)
    flat[flat.size // 2] -= math.fsum(list(flat) + [-1.0])
    return w


def blur_table_longdouble(kind, K, s1=1.0, s2=1.0, theta=0.0, beta=1.0, cutoff=1.0):
    """A second evaluation of the same table in numpy.longdouble (J1 stays scipy's fp64), rounded to fp64 at the end: what
    the first one's own rounding is measured against."""
    L = np.longdouble
    r = K // 2
    yy, xx = np.mgrid[0:K, 0:K]
    x, y = (xx - r).astype(L), (yy - r).astype(L)
    if kind == "sinc":
        from scipy.special import j1
        rr = np.sqrt(x * x + y * y)
        safe = np.where(rr == 0, L(1), rr)
        w = L(cutoff) * j1((L(cutoff) * safe).astype(np.float64)).astype(L) / (2 * L(np.pi) * safe)
        w = np.where(rr == 0, L(cutoff) * L(cutoff) / (4 * L(np.pi)), w)
    else:
        c, s = np.cos(L(theta)), np.sin(L(theta))
        u, v = c * x + s * y, -s * x + c * y
        q = u * u / (L(s1) * L(s1)) + v * v / (L(s2) * L(s2))
        w = np.exp(-q / 2) if kind == "gauss" else np.exp(-(q ** L(beta)) / 2) if kind == "ggauss" else 1 / (1 + q ** L(beta))
    return (w / w.sum()).astype(np.float64)


# (kind, s1, s2, theta, beta, cutoff) at every K of TABLE_KS
TABLE_KS = (7, 13, 21)
TABLE_CASES = [("gauss", 1.3, 1.3, 0.0, 1.0, 0.0), ("gauss", 2.7, 0.6, 0.9, 1.0, 0.0), ("ggauss", 1.9, 1.9, 0.0, 0.7, 0.0),
               ("ggauss", 2.4, 1.1, -2.2, 3.6, 0.0), ("plateau", 1.6, 1.6, 0.0, 1.4, 0.0), ("plateau", 2.9, 0.8, 1.7, 1.9, 0.0),
               ("sinc", 0.0, 0.0, 0.0, 0.0, math.pi / 3 + 0.1), ("sinc", 0.0, 0.0, 0.0, 0.0, 2.6)]


# -- the Poisson table ------------------------------------------------------------------------------------------------
def poisson_cdf(peak=PEAK, kt=KT):
    """cdf[256][kt]: the running product pmf(k) = pmf(k - 1) * lambda / k under Neumaier's sum, clamped to 1, made
    non-decreasing, last column 1.0 -- srk_poisson_cdf_host's operations in its order."""
    out = np.zeros((256, kt), np.float64)
    for L in range(256):
        lam = float(L) * peak / 255.0
        pmf, prev, s, comp = math.exp(-lam), 0.0, 0.0, 0.0
        for k in range(kt):
            if k > 0:
                pmf = pmf * lam / float(k)
            t = s + pmf
            comp += (s - t) + pmf if abs(s) >= abs(pmf) else (pmf - t) + s
            s = t
            v = min(s + comp, 1.0)
            v = max(v, prev)
            out[L, k] = prev = v
        out[L, kt - 1] = 1.0
    return out


_CDF = []


def cdf():
    if not _CDF:
        _CDF.append(poisson_cdf())
    return _CDF[0]


# -- the noise --------------------------------------------------------------------------------------------------------
def _words(seed, idx, stage):
    """(the four words, lane) of generator index idx (uint64 array) under `seed` with `stage` in counter word 2."""
    q = idx >> np.uint64(2)
    x = R1.philox4x32_10((q & R1.M32, q >> np.uint64(32), np.full_like(q, stage), np.zeros_like(q)),
                         (seed & 0xffffffff, seed >> 32))
    return x, (idx & np.uint64(3)).astype(np.int64)


def noise2_pre(x, mode, gray, amount, table, seed, stage=0, color=True):
    """x uint8 [B, C, H, W] -> the fp64 values x + amount * (...) + 0.5 that are floored and clamped (a patch with mode off:
    x + 0.5)."""
    B, C, H, W = x.shape
    HW = H * W
    xf = x.astype(np.float64)
    pre = xf + 0.5
    e = np.arange(x.size, dtype=np.uint64).reshape(x.shape)
    pix = np.arange(HW, dtype=np.uint64).reshape(1, H, W)
    for b in range(B):
        m = int(mode[b])
        if m not in (GAUSS, POISSON):
            continue
        g = gray[b] != 0.0
        idx = np.broadcast_to(np.uint64(b * HW) + pix, (C, H, W)) if g else e[b]
        words, lane = _words(seed, np.ascontiguousarray(idx), stage)
        a = float(amount[b])
        if m == GAUSS:
            lanes = []
            for h in range(2):
                rad = np.sqrt(-2.0 * np.log(R1.unit(words[2 * h])))
                ang = (2.0 * np.pi) * R1.unit(words[2 * h + 1])
                lanes += [rad * np.cos(ang), rad * np.sin(ang)]
            z = np.choose(lane, lanes)
            pre[b] = (xf[b] + a * z) + 0.5
            continue
        if g and C == 3:
            lg = np.floor((x[b, 0].astype(np.int64) + x[b, 1] + x[b, 2]).astype(np.float64) / 3.0 + 0.5) if color else xf[b, 0]
            lg = np.broadcast_to(lg, (C, H, W))
        else:
            lg = xf[b]
        u = R1.unit(np.choose(lane, words))
        k = np.zeros((C, H, W), np.float64)
        li = lg.astype(np.int64)
        for level in np.unique(li):
            sel = li == level
            k[sel] = np.searchsorted(table[level], u[sel], side='left')    # the smallest k with u <= cdf[level][k]
        d = k * 255.0 / 256.0 - lg
        pre[b] = (xf[b] + a * d) + 0.5
    return pre


def noise2_margin(pre, mode):
    """The rounding margin of the patches under Gaussian noise.  Only they pass through a libm (log, sqrt, sin, cos), which
    the two sides may round differently; the Poisson arithmetic is IEEE products and sums of table entries and bytes,
    uncontracted on both sides, so even a value exactly on a boundary (amounts such as 3.0 make k * 255 / 256 terms land
    there) rounds the same way everywhere."""
    sel = np.asarray(mode) == GAUSS
    return margin(pre[sel]) if sel.any() else 1.0


def noise2(x, mode, gray, amount, table, seed, stage=0, color=True):
    return np.clip(np.floor(noise2_pre(x, mode, gray, amount, table, seed, stage, color)), 0.0, 255.0).astype(np.uint8)


# -- the unsharp mask -------------------------------------------------------------------------------------------------
def usm_table(K=51, sigma=0.0):
    if sigma <= 0.0:
        sigma = 0.3 * ((K - 1) * 0.5 - 1.0) + 0.8
    c = K // 2
    g = np.array([math.exp(-(float(i - c) * float(i - c)) / (2.0 * (sigma * sigma))) for i in range(K)], np.float64)
    return _normalised(g)


def _sep_blur(a, g):
    """a fp64 [..., H, W]: rows then columns, taps in index order from 0.0, reflect-101."""
    K = len(g)
    r = K // 2
    H, W = a.shape[-2:]
    assert H > r and W > r
    pad = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode='reflect')
    rows = np.zeros(pad.shape[:-1] + (W,), np.float64)
    for t in range(K):
        rows = rows + g[t] * pad[..., :, t:t + W]
    out = np.zeros(a.shape, np.float64)
    for t in range(K):
        out = out + g[t] * rows[..., t:t + H, :]
    return out


def usm_parts(x, g, weight=0.5, threshold=10.0):
    """x uint8 [B, C, H, W] -> (pre, resid): the fp64 values clamp(...) + 0.5 that are floored, and |R| - threshold."""
    p = x.astype(np.float64)
    res = p - _sep_blur(p, g)
    mask = (np.abs(res) > threshold).astype(np.float64)
    soft = _sep_blur(mask, g)
    sharp = np.clip(p + weight * res, 0.0, 255.0)
    return np.clip(soft * sharp + (1.0 - soft) * p, 0.0, 255.0) + 0.5, np.abs(res) - threshold


def usm(x, g, weight=0.5, threshold=10.0):
    return np.floor(usm_parts(x, g, weight, threshold)[0]).astype(np.uint8)


def margin(pre):
    """Smallest distance of the values about to be floored from an integer."""
    return float(np.abs(pre - np.round(pre)).min())


# -- Pillow -----------------------------------------------------------------------------------------------------------
def pil_resize(planes, oh, ow, filt):
    """Image.resize((ow, oh), filt) of every 8-bit plane of [..., H, W]."""
    from PIL import Image
    flat = planes.reshape((-1,) + planes.shape[-2:])
    out = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(pl), "L").resize((ow, oh), filt), dtype=np.uint8)
                    for pl in flat])
    return out.reshape(planes.shape[:-2] + (oh, ow))


# -- case tables (the CPU guard and the GPU tests share them) ----------------------------------------------------------
# (name, image seed, shape, mode, gray, amount per patch, noise seed, stage, color)
NOISE2_CASES = [
    ("gauss_colour_rgb", 31, (3, 3, 5, 7), [1, 1, 1], [0, 0, 0], [0.0, 1.0, 30.0], 0x0123456789abcdef, 0, True),
    ("gauss_gray_rgb", 32, (3, 3, 5, 7), [1, 1, 0], [1, 1, 1], [1.0, 30.0, 9.0], 0xfedcba9876543210, 1, True),
    ("poisson_colour_rgb", 33, (3, 3, 5, 7), [2, 2, 2], [0, 0, 0], [0.0, 0.05, 3.0], 0x9e3779b97f4a7c15, 2, True),
    ("poisson_gray_rgb", 34, (3, 3, 5, 7), [2, 0, 2], [1, 1, 1], [0.05, 1.0, 3.0], 0x5851f42d4c957f2d, 1, True),
    ("poisson_gray_ycc", 35, (3, 3, 5, 7), [2, 2, 2], [1, 0, 1], [2.5, 1.0, 0.05], 0x14057b7ef767814f, 2, False),
    ("mixed_rgb", 36, (3, 3, 5, 7), [1, 0, 2], [1, 0, 0], [25.0, 5.0, 2.5], 0x2545f4914f6cdd1d, 2, True),
    ("gauss_y", 37, (2, 1, 16, 16), [1, 1], [0, 1], [1.0, 30.0], 0xd1342543de82ef95, 1, False),
    ("poisson_y", 38, (2, 1, 16, 16), [2, 2], [0, 1], [3.0, 0.05], 0xaf251af3b0f025b5, 2, False),
    ("mixed_y", 39, (2, 1, 16, 16), [0, 2], [0, 0], [4.0, 1.5], 0xb564ef22ec7aece5, 1, False),
    ("odd_batch", 40, (5, 3, 33, 31), [1, 2, 0, 2, 1], [0, 1, 0, 0, 1], [12.0, 2.0, 1.0, 0.7, 20.0], 0x27bb2ee687b0b0fd, 2, True),
]
NOISE2_CPU = [c[0] for c in NOISE2_CASES if c[0] != "odd_batch"]


def noise2_case(name):
    for n, iseed, shape, mode, gray, amount, seed, stage, color in NOISE2_CASES:
        if n == name:
            f = lambda v: np.asarray(v, np.float64)
            return R1.image(iseed, shape), f(mode), f(gray), f(amount), seed, stage, color
    raise KeyError(name)


# (name, image seed, shape, K, weight, threshold)
USM_CASES = [
    ("radius_25", 41, (2, 3, 27, 40), 51, 0.5, 10.0),
    ("y_64", 42, (1, 1, 64, 64), 51, 0.5, 10.0),
    ("k5_tiny", 43, (1, 3, 3, 3), 5, 0.5, 10.0),
    ("odd_batch", 44, (5, 3, 33, 31), 51, 0.5, 10.0),
]
USM_CPU = [c[0] for c in USM_CASES if c[0] != "odd_batch"]


def usm_case(name):
    for n, iseed, shape, K, weight, threshold in USM_CASES:
        if n == name:
            return R1.image(iseed, shape), usm_table(K), weight, threshold
    raise KeyError(name)


# BOX resize: (image seed, (C, H, W), (oh, ow))
BOX_CASES = [(51, (3, 48, 48), (7, 7)), (51, (3, 48, 48), (19, 30)), (51, (3, 48, 48), (72, 72)), (51, (3, 48, 48), (48, 48)),
             (52, (1, 11, 13), (5, 6))]

# signed and plateau tables through srk_blur_u8: (image seed, shape) x (kind, K, s1, s2, theta, beta, cutoff)
BLUR2_SHAPES = [(61, (2, 3, 11, 23)), (62, (1, 3, 48, 48))]
BLUR2_TABLES = [("sinc", 7, 0, 0, 0, 0, 2.1), ("sinc", 21, 0, 0, 0, 0, 0.9), ("plateau", 7, 1.4, 0.7, 0.6, 1.5, 0),
                ("plateau", 21, 2.8, 2.8, 0.0, 1.1, 0)]


# -- the draws of data.Degradation2 and the whole chain ----------------------------------------------------------------
DEFAULTS = dict(kernel_sizes=tuple(range(7, 22, 2)), kernel_sizes2=tuple(range(7, 22, 2)),
                kernel_prob=(.45, .25, .12, .03, .12, .03), kernel_prob2=(.45, .25, .12, .03, .12, .03),
                sinc_prob=.1, sinc_prob2=.1, blur_sigma=(0.2, 3.0), blur_sigma2=(0.2, 1.5),
                betag_range=(0.5, 4.0), betag_range2=(0.5, 4.0), betap_range=(1.0, 2.0), betap_range2=(1.0, 2.0),
                second_blur_prob=0.8, resize_prob=(.2, .7, .1), resize_prob2=(.3, .4, .3),
                resize_range=(0.15, 1.5), resize_range2=(0.3, 1.2), gaussian_noise_prob=.5, gaussian_noise_prob2=.5,
                noise_range=(1.0, 30.0), noise_range2=(1.0, 25.0), poisson_scale_range=(0.05, 3.0),
                poisson_scale_range2=(0.05, 2.5), gray_noise_prob=.4, gray_noise_prob2=.4, jpeg_range=(30, 95),
                jpeg_range2=(30, 95), final_sinc_prob=0.8)


def _cutoff(rng, K):
    return rng.uniform(math.pi / 3 if K < 13 else math.pi / 5, math.pi)


def _kernel(cfg, rng, sfx):
    K = rng.choice(cfg['kernel_sizes' + sfx])
    if rng.random() < cfg['sinc_prob' + sfx]:
        return ("sinc", K, 0.0, 0.0, 0.0, 0.0, _cutoff(rng, K))
    r, acc, kind = rng.random(), 0.0, len(KINDS) - 1
    for i, pk in enumerate(cfg['kernel_prob' + sfx]):
        acc += pk
        if r < acc:
            kind = i
            break
    name, aniso = KINDS[kind]
    lo, hi = cfg['blur_sigma' + sfx]
    s1 = rng.uniform(lo, hi)
    s2, theta = (rng.uniform(lo, hi), rng.uniform(-math.pi, math.pi)) if aniso else (s1, 0.0)
    beta = 1.0
    if name == "ggauss":
        beta = rng.uniform(*cfg['betag_range' + sfx])
    elif name == "plateau":
        beta = rng.uniform(*cfg['betap_range' + sfx])
    return (name, K, s1, s2, theta, beta, 0.0)


def _resize(cfg, rng, sfx):
    up, down, _ = cfg['resize_prob' + sfx]
    lo, hi = cfg['resize_range' + sfx]
    r = rng.random()
    s = rng.uniform(1.0, hi) if r < up else (rng.uniform(lo, 1.0) if r < up + down else 1.0)
    return s, rng.choice(FILTERS)


def _noise(cfg, rng, batch, sfx):
    gauss = rng.random() < cfg['gaussian_noise_prob' + sfx]
    lo, hi = cfg[('noise_range' if gauss else 'poisson_scale_range') + sfx]
    amount, gray = [], []
    for _ in range(batch):
        amount.append(rng.uniform(lo, hi))
        gray.append(float(rng.random() < cfg['gray_noise_prob' + sfx]))
    return dict(mode=np.full(batch, float(GAUSS if gauss else POISSON)), gray=np.asarray(gray, np.float64),
                amount=np.asarray(amount, np.float64), seed=rng.getrandbits(64))


def _tables(specs):
    K = max([s[1] for s in specs if s is not None] + [7])
    return np.stack([R1.centred(blur_table(*s) if s is not None else R1.delta(7), K) for s in specs])


def draw(batch, rng=random, **overrides):
    """data.Degradation2.draw restated: the same calls on `rng` in the same order; the kernels also as their specs."""
    cfg = dict(DEFAULTS, **overrides)
    p = {}
    p['spec1'] = [_kernel(cfg, rng, '') for _ in range(batch)]
    p['s1'], p['f1'] = _resize(cfg, rng, '')
    p['n1'] = _noise(cfg, rng, batch, '')
    p['q1'] = np.array([rng.randint(*cfg['jpeg_range']) for _ in range(batch)], np.float64)
    p['spec2'] = [_kernel(cfg, rng, '2') if rng.random() < cfg['second_blur_prob'] else None for _ in range(batch)]
    p['s2'], p['f2'] = _resize(cfg, rng, '2')
    p['n2'] = _noise(cfg, rng, batch, '2')
    p['resize_first'] = rng.random() < 0.5
    p['f3'] = rng.choice(FILTERS)
    p['spec3'] = []
    for _ in range(batch):
        if rng.random() < cfg['final_sinc_prob']:
            K = rng.choice(cfg['kernel_sizes2'])
            p['spec3'].append(("sinc", K, 0.0, 0.0, 0.0, 0.0, _cutoff(rng, K)))
        else:
            p['spec3'].append(None)
    p['q2'] = np.array([rng.randint(*cfg['jpeg_range2']) for _ in range(batch)], np.float64)
    for i in '123':
        p['k' + i] = _tables(p['spec' + i])
    return p


def chain(patches, p, lr_hw, color=True, subsampling=1):
    """patches uint8 [B, C, H, W] under the drawn p -> (lr fp32 [B, C, lh, lw], the smallest rounding margin met)."""
    B, C, H, W = patches.shape
    lh, lw = lr_hw
    guard = [1.0]
    x = patches

    def blur(x, w):
        K = w.shape[1]
        if not (w[:, K // 2, K // 2] != 1.0).any():
            return x
        pre = R1.blur_pre(x, w)
        guard.append(margin(pre))
        return np.floor(pre).astype(np.uint8)

    def resize(x, oh, ow, filt):
        oh, ow = max(1, oh), max(1, ow)
        return x if (oh, ow) == x.shape[2:] else pil_resize(x, oh, ow, filt)

    def noise(x, n, stage):
        pre = noise2_pre(x, n['mode'], n['gray'], n['amount'], cdf(), n['seed'], stage, color)
        guard.append(noise2_margin(pre, n['mode']))
        return np.clip(np.floor(pre), 0.0, 255.0).astype(np.uint8)

    def jpeg(x, q):
        return J.jpeg(x, q, subsampling, 1 if color else 0)

    x = jpeg(noise(resize(blur(x, p['k1']), int(H * p['s1']), int(W * p['s1']), p['f1']), p['n1'], 1), p['q1'])
    x = noise(resize(blur(x, p['k2']), int(lh * p['s2']), int(lw * p['s2']), p['f2']), p['n2'], 2)
    if p['resize_first']:
        x = jpeg(blur(resize(x, lh, lw, p['f3']), p['k3']), p['q2'])
    else:
        x = blur(resize(jpeg(x, p['q2']), lh, lw, p['f3']), p['k3'])
    return x.astype(np.float32) / np.float32(255.0), min(guard)


# -- the tiny image folder and the end-to-end replay -------------------------------------------------------------------
E2E = dict(crop_size=48, scale_factor=4, batch=4, overrides=dict(resize_range=(0.5, 1.5)))
E2E_SEEDS = (1, 2, 3, 4, 5, 6)
FOLDER_SIZES = [(96, 80), (72, 88), (100, 100), (84, 76)]
TEST_SEED = 7


def make_folder(folder):
    return R1.make_folder(folder, sizes=FOLDER_SIZES, seed=71)


def coverage(ps):
    """What a set of drawn batches exercises: the things the GPU test asserts to be covered."""
    seen = set()
    for p in ps:
        seen.add("resize_first" if p['resize_first'] else "jpeg_first")
        for n in (p['n1'], p['n2']):
            seen.add("gauss" if n['mode'][0] == GAUSS else "poisson")
            if n['gray'].any():
                seen.add("gray")
        if any(s is None for s in p['spec2']):
            seen.add("no_second_blur")
        seen.update("filter%d" % f for f in (p['f1'], p['f2'], p['f3']))
    return seen


WANTED = {"resize_first", "jpeg_first", "gauss", "poisson", "gray", "no_second_blur", "filter2", "filter3", "filter4"}


def replay_batch(folder, seed, is_gray=False, usm_on=False):
    """The first batch of an unshuffled PatchLoader over TrainDatasetFromFolder([folder], degrade=Degradation2(**E2E
    ['overrides']), usm=usm_on) after random.seed(seed), on the CPU: the patches from the oracle restatement of the
    reference's dataset, the chain from this module.  A dict with lr, hr, bc (fp32), the drawn p and the guard."""
    import torch
    from oracle import dataset_pil as O
    crop, sf, B = E2E['crop_size'], E2E['scale_factor'], E2E['batch']
    ora = O.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=crop, scale_factor=sf)
    random.seed(seed)
    hr = torch.stack([ora[i][1] for i in range(B)]).numpy()
    patches = np.round(hr * np.float32(255.0)).astype(np.uint8)
    assert (patches.astype(np.float32) / np.float32(255.0) == hr).all()
    guard = 1.0
    if usm_on:
        pre, resid = usm_parts(patches, usm_table())
        guard = min(margin(pre), float(np.abs(resid).min()))
        patches = np.floor(pre).astype(np.uint8)
        hr = patches.astype(np.float32) / np.float32(255.0)
    p = draw(B, random, **E2E['overrides'])
    lr, g = chain(patches, p, (crop // sf, crop // sf), color=not is_gray)
    return dict(lr=lr, hr=hr, bc=R1.bicubic_of_lr(lr, crop, crop), p=p, guard=min(guard, g))


def test_item(hwc, sf, seed, index, is_gray=False):
    """TestDatasetFromFolder(degrade2=(Degradation2(**E2E['overrides']), seed))'s lr of a decoded image [H, W, C]."""
    h, w, c = hwc.shape
    lr_hw = ((h - h % sf) // sf, (w - w % sf) // sf)
    p = draw(1, random.Random("degrade2:%d:%d" % (seed, index)), **E2E['overrides'])
    lr, g = chain(np.ascontiguousarray(hwc.transpose(2, 0, 1))[None], p, lr_hw, color=not is_gray)
    return lr[0], g
