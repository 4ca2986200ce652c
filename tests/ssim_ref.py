"""What tests/test_ssim_cpu.py and tests/test_ssim_gpu.py share: an fp64 numpy restatement of SSIM (Wang, Bovik, Sheikh,
Simoncelli 2004, as ssim_index.m computes it), the three evaluation domains via numpy and Pillow, and the case table.
Nothing here uses the package under test."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _valid_filter(a):
    """11 x 11 separable Gaussian at the valid positions of [..., H, W] (plain slicing, fp64)."""
    g = window()
    mw, mh = a.shape[-1] - 10, a.shape[-2] - 10
    hx = sum(g[k] * a[..., :, k:k + mw] for k in range(11))
    return sum(g[k] * hx[..., k:k + mh, :] for k in range(11))


def ssim_map(x, y, L=1.0):
    """The SSIM map of fp64 planes [..., H, W] with dynamic range L."""
    x, y = np.asarray(x, np.float64) / L, np.asarray(y, np.float64) / L
    mx, my = _valid_filter(x), _valid_filter(y)
    vx, vy, cov = _valid_filter(x * x) - mx * mx, _valid_filter(y * y) - my * my, _valid_filter(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def quantise(v):
    """ToPILImage after clamp(0, 1): fp32 product, truncation; NaN -> 0."""
    v = np.asarray(v, np.float32)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    return (v * np.float32(255.0)).astype(np.uint8)


def pillow_luma(u8_nchw):
    """[N,3,H,W] bytes -> [N,1,H,W] bytes: the Y of Image.fromarray(picture).convert('YCbCr')."""
    from PIL import Image
    out = [np.asarray(Image.fromarray(np.ascontiguousarray(p.transpose(1, 2, 0))).convert('YCbCr'))[:, :, 0] for p in u8_nchw]
    return np.stack(out)[:, None]


def planes(pred, gt, domain):
    """What enters the moments: (x, y, L) as fp64 [N,P,H,W]."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    if domain == 'float':
        p = np.where(np.isnan(pred), np.float32(0), np.clip(pred, np.float32(0), np.float32(1)))
        return p.astype(np.float64), gt.astype(np.float64), 1.0
    a, b = quantise(pred), quantise(gt)
    if domain == 'y8' and a.shape[1] == 3:
        a, b = pillow_luma(a), pillow_luma(b)
    else:
        assert domain == 'u8' or a.shape[1] == 1
    return a.astype(np.float64), b.astype(np.float64), 255.0


def crop(a, shave):
    return a[..., shave:a.shape[-2] - shave, shave:a.shape[-1] - shave]


def ssim_ref(pred, gt, shave=0, domain='float'):
    """(ssim, psnr, mse) of [N,C,H,W] fp32 arrays in fp64: the definition the device kernel and srk_ssim_host follow."""
    x, y, L = planes(pred, gt, domain)
    x, y = crop(x, shave), crop(y, shave)
    mse = float(np.mean(((x - y) / L) ** 2))
    return float(ssim_map(x, y, L).mean()), (100.0 if mse == 0 else 10 * np.log10(1 / mse)), mse


def seeded_picture():
    """The sanity pin of the restatement: (pred, gt) [97, 131] fp64 in [0, 1]; SSIM 0.917089."""
    rng = np.random.RandomState(7)
    yy, xx = np.mgrid[0:97, 0:131]
    s = 0.5 + 0.3 * np.sin(xx / 9) * np.cos(yy / 13) + 0.15 * np.sin((xx + yy) / 3.1)
    gt = np.clip(s + 0.02 * rng.randn(97, 131), 0, 1)
    pred = np.clip(gt + 0.03 * rng.randn(97, 131), 0, 1)
    return pred, gt


def cases():
    """name -> (pred, gt), fp32 [N,C,H,W].  Textured, quantised, noise against noise (negative map values), bright and
    flat, constant, identical; one position (11 x 11), one row of positions (11 x 300), 97 x 131, N = 2 with C = 3 and
    predictions that leave [0, 1] and hold a NaN."""
    rng = np.random.RandomState(11)
    pred, gt = seeded_picture()
    out = {}
    out["picture"] = (pred[None, None], gt[None, None])
    out["picture_8bit"] = (quantise(pred)[None, None] / np.float32(255), quantise(gt)[None, None] / np.float32(255))
    out["noise"] = (rng.rand(1, 1, 97, 131), rng.rand(1, 1, 97, 131))
    out["bright_flat"] = (0.97 + 1e-3 * rng.randn(1, 1, 97, 131), 0.97 + 1e-3 * rng.randn(1, 1, 97, 131))
    out["constant"] = (np.full((1, 1, 40, 50), 0.9), np.full((1, 1, 40, 50), 0.8))
    same = rng.rand(1, 3, 33, 47)
    out["identical"] = (same, same.copy())
    out["one_position"] = (rng.rand(1, 1, 11, 11), rng.rand(1, 1, 11, 11))
    g = rng.rand(1, 3, 11, 300)
    out["one_row"] = (g + 0.05 * rng.randn(*g.shape), g)
    yy, xx = np.mgrid[0:97, 0:131]
    g = np.stack([0.5 + 0.4 * np.sin(xx / (5.0 + c)) * np.cos(yy / (7.0 + n)) for n in range(2) for c in range(3)])
    g = np.clip(g.reshape(2, 3, 97, 131) + 0.02 * rng.randn(2, 3, 97, 131), 0, 1)
    p = g + 0.08 * rng.randn(*g.shape)          # leaves [0, 1]: the clamp is part of every domain
    p[1, 2, 50, 60] = np.nan                     # counts as 0
    out["batch_rgb"] = (p, g)
    return {k: (np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32))
            for k, (a, b) in out.items()}


SHAVES = (0, 4, 8)
DOMAINS = ('float', 'u8', 'y8')
LAYOUTS = ('nchw', 'channels_last', 'cropped_view')


def combos():
    """Every (case, domain, shave) of the table that leaves at least the window."""
    for name, (p, g) in cases().items():
        for domain in DOMAINS:
            for shave in SHAVES:
                if min(p.shape[-2:]) - 2 * shave >= 11:
                    yield name, p, g, domain, shave
