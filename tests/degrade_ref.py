"""fp64 numpy restatement of the training degradations (include/srk.h): LR = (HR * k) shrunk + n.

Philox4x32-10, the Box-Muller normals, the anisotropic Gaussian tables, the blur by explicit tap loops over
np.pad(..., mode='reflect'), the noise, the draws from Python's `random`, and the whole of
TrainDatasetFromFolder.finish with Pillow's Image.resize(..., BICUBIC) per plane in the middle.  Test infrastructure
only; nothing here runs in the package.  CASES is the table the CPU guard and the GPU tests share."""
import math
import random

import numpy as np

MAX_K = 21
M32 = np.uint64(0xffffffff)


# -- Philox4x32-10 and the normals ------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints.  Returns the four output words as uint64 arrays
    holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in counter]
    k0, k1 = np.uint64(key[0] & 0xffffffff), np.uint64(key[1] & 0xffffffff)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def unit(x):
    return (x.astype(np.float64) + 0.5) * 2.0 ** -32


def normals(seed, first_elem, n):
    """The fp64 normals of elements first_elem .. first_elem + n - 1 under `seed`."""
    e = np.arange(first_elem, first_elem + n, dtype=np.uint64)
    q = e >> np.uint64(2)
    zero = np.zeros_like(q)
    x = philox4x32_10((q & M32, q >> np.uint64(32), zero, zero), (seed & 0xffffffff, seed >> 32))
    lanes = []
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(unit(x[2 * h])))
        ang = (2.0 * np.pi) * unit(x[2 * h + 1])
        lanes += [rad * np.cos(ang), rad * np.sin(ang)]
    lane = (e & np.uint64(3)).astype(np.int64)
    return np.choose(lane, lanes)


# -- blur tables -------------------------------------------------------------------------------------------------------
def kernel_size(s1, s2):
    return min(MAX_K, 2 * int(math.ceil(3 * max(s1, s2))) + 1)


def blur_weights(s1, s2, theta, K):
    """The normalised K x K table, row-major (i, j) = (y + r, x + r); scalar fp64 arithmetic in the documented order."""
    r = K // 2
    c, s = math.cos(theta), math.sin(theta)
    w = np.zeros((K, K), np.float64)
    for i in range(K):
        for j in range(K):
            x, y = float(j - r), float(i - r)
            u, v = c * x + s * y, -s * x + c * y
            w[i, j] = math.exp(-0.5 * (u * u / (s1 * s1) + v * v / (s2 * s2)))
    # the fp64 sum, correctly rounded (the library: a compensated row-major sum).  A plain running sum of 441 terms is
    # off by up to ~1.5e-15 of the total, and the normalised table's sum would be off from 1 by as much.
    return w / math.fsum(w.ravel())


def delta(K):
    w = np.zeros((K, K), np.float64)
    w[K // 2, K // 2] = 1.0
    return w


def centred(w, K):
    """The table w (k x k, k <= K) centred among zeros in K x K."""
    k = w.shape[0]
    out = np.zeros((K, K), np.float64)
    o = (K - k) // 2
    out[o:o + k, o:o + k] = w
    return out


# -- the two operators ------------------------------------------------------------------------------------------------
def blur_pre(p, w):
    """p uint8 [B, C, H, W], w fp64 [B, K, K] -> the fp64 values clamp(sum, 0, 255) + 0.5 that are floored."""
    B, C, H, W = p.shape
    K = w.shape[1]
    r = K // 2
    assert H > r and W > r
    pad = np.pad(p.astype(np.float64), ((0, 0), (0, 0), (r, r), (r, r)), mode='reflect')
    acc = np.zeros(p.shape, np.float64)
    for b in range(B):
        for i in range(K):
            for j in range(K):     # row-major taps, one product and one addition each
                acc[b] = acc[b] + w[b, i, j] * pad[b, :, i:i + H, j:j + W]
    return np.clip(acc, 0.0, 255.0) + 0.5


def blur(p, w):
    return np.floor(blur_pre(p, w)).astype(np.uint8)


def noise_pre(x, sigma, seed):
    """x uint8 [B, ...], sigma fp64 [B] -> the fp64 values x + sigma * z + 0.5 that are floored."""
    B = x.shape[0]
    z = normals(seed, 0, x.size).reshape(x.shape)
    s = np.asarray(sigma, np.float64).reshape((B,) + (1,) * (x.ndim - 1))
    return x.astype(np.float64) + s * z + 0.5


def noise(x, sigma, seed):
    return np.clip(np.floor(noise_pre(x, sigma, seed)), 0.0, 255.0).astype(np.float32) / np.float32(255.0)


# -- draws and the whole finish ---------------------------------------------------------------------------------------
def draw(batch, blur_prob, blur_sigma, noise_sigma):
    """Consumes Python's `random` in the documented order.  Returns (weights [B, K, K], sigma [B], seed)."""
    lo, hi = blur_sigma
    nlo, nhi = noise_sigma
    tables, sigma = [], []
    for _ in range(batch):
        if random.random() < blur_prob:
            s1, s2 = random.uniform(lo, hi), random.uniform(lo, hi)
            th = random.uniform(0, math.pi)
            tables.append(blur_weights(s1, s2, th, kernel_size(s1, s2)))
        else:
            tables.append(None)
        sigma.append(random.uniform(nlo, nhi) if nhi > 0 else 0.0)
    seed = random.getrandbits(64) if nhi > 0 else 0
    K = max([t.shape[0] for t in tables if t is not None] + [3])
    w = np.stack([centred(t if t is not None else delta(3), K) for t in tables])
    return w, np.asarray(sigma, np.float64), seed


def pil_resize(planes, oh, ow):
    """Image.resize((ow, oh), BICUBIC) of every 8-bit plane of [..., H, W]."""
    from PIL import Image
    flat = planes.reshape((-1,) + planes.shape[-2:])
    out = np.stack([np.asarray(Image.fromarray(pl, "L").resize((ow, oh), Image.BICUBIC), dtype=np.uint8) for pl in flat])
    return out.reshape(planes.shape[:-2] + (oh, ow))


def bicubic_of_lr(lr, oh, ow):
    """ToPILImage -> resize -> ToTensor of the fp32 batch (oracle/dataset_pil.py: mul(255).byte(), /255)."""
    u8 = (lr * np.float32(255.0)).astype(np.uint8)
    return pil_resize(u8, oh, ow).astype(np.float32) / np.float32(255.0)


def apply(patches, w, sigma, seed, lr_sz):
    """patches uint8 [B, C, crop, crop] -> the degraded fp32 lr [B, C, lr_sz, lr_sz]."""
    return noise(pil_resize(blur(patches, w), lr_sz, lr_sz), sigma, seed)


def finish(patches, w, sigma, seed, lr_sz):
    """(lr, bc) of the degraded branch of TrainDatasetFromFolder.finish."""
    lr = apply(patches, w, sigma, seed, lr_sz)
    return lr, bicubic_of_lr(lr, patches.shape[2], patches.shape[3])


# -- the case table ---------------------------------------------------------------------------------------------------
def image(seed, shape):
    """Seeded 8-bit planes with structure: a smooth ramp, noise and hard edges."""
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    base = 96.0 + 80.0 * np.sin(xx / 3.1 + seed) * np.cos(yy / 4.3)
    a = base[None, None] + rs.normal(0, 40, shape)
    a[:, :, H // 3, :] = 255
    a[:, :, :, W // 2] = 0
    return np.clip(a, 0, 255).astype(np.uint8)


def tables(seed, B, K, kinds):
    """B tables padded to K x K; kinds[b]: 'full' (the widest table K allows), 'delta', or an odd size below K."""
    rs = random.Random(seed)
    out = []
    for b in range(B):
        kind = kinds[b % len(kinds)]
        if kind == 'delta':
            out.append(centred(delta(3), K))
            continue
        k = K if kind == 'full' else int(kind)
        if kind == 'full':          # wide for its size (the kernel takes any table): every tap carries weight
            s1, s2 = rs.uniform(0.12, 0.19) * k, rs.uniform(0.06, 0.19) * k
        else:                       # a table of the size its sigmas ask for: 2 * ceil(3 s) + 1 == k
            s1, s2 = rs.uniform((k - 3) / 6.0 + 0.01, (k - 1) / 6.0), rs.uniform(0.2, (k - 1) / 6.0)
            assert kernel_size(s1, s2) == k
        out.append(centred(blur_weights(s1, s2, rs.uniform(0, math.pi), k), K))
    return np.stack(out)


# (name, image seed, (B, C, H, W), K, kinds of the B tables)
BLUR_CASES = [
    ("halo_max", 11, (1, 1, 11, 11), 21, ['full']),
    ("three_tables", 12, (3, 3, 24, 24), 21, ['full', 'delta', 'full']),
    ("ragged", 13, (2, 3, 37, 29), 7, ['full']),
    ("k3_wide", 14, (2, 1, 33, 65), 3, ['full']),
    ("loader_patch", 15, (1, 3, 128, 128), 21, ['full']),
    ("k7_beside_k21", 16, (2, 3, 24, 40), 21, [7, 'full']),
]


def blur_case(name):
    for n, seed, shape, K, kinds in BLUR_CASES:
        if n == name:
            return image(seed, shape), tables(seed + 100, shape[0], K, kinds)
    raise KeyError(name)


# (name, image seed, (B, C, h, w), sigma per patch, noise seed)
NOISE_CASES = [
    ("short_group", 21, (1, 1, 3, 5), [7.5], 0x0123456789abcdef),
    ("three_sigmas", 22, (3, 3, 8, 8), [0.0, 2.5, 25.0], 0xfedcba9876543210),
    ("loader_lr", 23, (16, 3, 32, 32), [10.0 * (b + 1) / 16 for b in range(16)], 0x9e3779b97f4a7c15),
]


STAT_SEED = 0x5eed5eed5eed5eed   # identities and statistics of the noise


def noise_case(name):
    for n, seed, shape, sigma, nseed in NOISE_CASES:
        if n == name:
            return image(seed, shape), np.asarray(sigma, np.float64), nseed
    raise KeyError(name)


def boundary_distance(pre):
    """Smallest distance of the values about to be floored from an integer."""
    return float(np.abs(pre - np.round(pre)).min())


# -- the tiny image folder and the end-to-end replay ---------------------------------------------------------------------
E2E = dict(crop_size=32, scale_factor=4, batch=2, seed=1,
           degradation=dict(blur_prob=0.5, blur_sigma=(0.4, 3.5), noise_sigma=(1.0, 12.0)))
TEST_DEGRADE = (1.2, 2.0, math.radians(30.0), 5.0)
FOLDER_SIZES = [(64, 48), (40, 56), (72, 72), (50, 44)]


def make_folder(folder, sizes=FOLDER_SIZES, seed=5):
    import os
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, (w, h) in enumerate(sizes):
        a = image(seed + i, (1, 3, h, w))[0].transpose(1, 2, 0)
        Image.fromarray(np.ascontiguousarray(a), "RGB").save(os.path.join(folder, "img_%02d.png" % i))
    return folder


def replay_batches(folder, n_batches, is_gray=False):
    """The first n_batches of an unshuffled PatchLoader over TrainDatasetFromFolder([folder], degrade=Degradation(**E2E
    ['degradation'])) after random.seed(E2E['seed']), on the CPU: the patches come from the oracle restatement of the
    reference's dataset (its hr item is the 8-bit patch / 255), the degradation from this module.  Per batch a dict with
    lr, hr, bc (fp32) and the two guard distances."""
    import torch
    from oracle import dataset_pil as O
    ora = O.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=E2E['crop_size'], scale_factor=E2E['scale_factor'])
    d, B, lr_sz = E2E['degradation'], E2E['batch'], E2E['crop_size'] // E2E['scale_factor']
    random.seed(E2E['seed'])
    out = []
    for k in range(n_batches):
        hr = torch.stack([ora[i][1] for i in range(k * B, (k + 1) * B)]).numpy()
        patches = np.round(hr * np.float32(255.0)).astype(np.uint8)
        assert (patches.astype(np.float32) / np.float32(255.0) == hr).all()
        w, sigma, seed = draw(B, d['blur_prob'], d['blur_sigma'], d['noise_sigma'])
        q = pil_resize(blur(patches, w), lr_sz, lr_sz)
        lr, bc = finish(patches, w, sigma, seed, lr_sz)
        out.append(dict(lr=lr, hr=hr, bc=bc, blurred=int((w[:, w.shape[1] // 2, w.shape[1] // 2] != 1.0).sum()),
                        blur_guard=boundary_distance(blur_pre(patches, w)),
                        noise_guard=boundary_distance(noise_pre(q, sigma, seed))))
    return out


def item_lr_of_test_set(hwc, sf, degrade, index):
    """TestDatasetFromFolder's degraded lr of a decoded image [H, W, C]: fixed table, noise seed = the image's index."""
    s1, s2, th, ns = degrade
    h, w, c = hwc.shape
    lr_h, lr_w = (h - h % sf) // sf, (w - w % sf) // sf
    planes = np.ascontiguousarray(hwc.transpose(2, 0, 1))[None]
    q = blur(planes, blur_weights(s1, s2, th, kernel_size(s1, s2))[None])
    return noise(pil_resize(q, lr_h, lr_w), [ns], index)[0]
