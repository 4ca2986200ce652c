"""NIQE (Mittal, Soundararajan, Bovik 2013) restated in numpy / scipy, fp64: the yardstick of tests/test_niqe_cpu.py (the host
twin) and tests/test_niqe_gpu.py (the kernels).  The definition is the one pinned in include/srk.h; it follows BasicSR's
calculate_niqe as remembered, not as checked against its file, so this restatement -- not BasicSR -- is the reference.

Also the case table: seeded pictures (Gaussian-filtered noise on a ramp, so the MSCN maps have structure) at the smallest
shapes that reach every path of the kernel."""
import functools

import numpy as np
from scipy import ndimage, special

GAM = np.arange(0.2, 10.001, 0.001)
R_GAM = special.gamma(2.0 / GAM) ** 2 / (special.gamma(1.0 / GAM) * special.gamma(3.0 / GAM))
SHRINK = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))

FEATURE_TOL = 1e-9    # |dev - ref| <= FEATURE_TOL * max(1, |ref|), element-wise; NaN positions identical
SCORE_RTOL = 1e-6
COND_MAX = 1e7


def window():
    i = np.arange(7)
    g = np.exp(-(i - 3.0) ** 2 / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def cubic(x):
    """Keys' cubic convolution kernel, a = -0.5 (MATLAB's bicubic)."""
    x = np.abs(x)
    return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1,
                    np.where(x < 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))


def shrink_weights_from_formula():
    """MATLAB's antialiased kernel at scale 1/2 is cubic(x / 2) / 2; output i sits at input coordinate 2 i + 0.5 and reads
    2 i - 3 .. 2 i + 4."""
    d = np.arange(-3, 5) - 0.5
    return cubic(d / 2.0) / 2.0


def quantise(img):
    """[C,H,W] float32 -> the bytes of (uint8)(clamp(v, 0, 1) * 255.0f); uint8 is taken as it is."""
    if img.dtype == np.uint8:
        return img
    v = np.clip(img.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(255.0)
    return v.astype(np.uint8)


def luma(u8):
    """[C,H,W] bytes -> the fp64 plane: BT.601 studio range for three channels, the byte itself for one."""
    b = u8.astype(np.float64)
    if b.shape[0] == 1:
        return b[0]
    return np.rint(16.0 + (65.481 * b[0] + 128.553 * b[1] + 24.966 * b[2]) / 255.0)


def crop(plane, shave, block):
    h, w = plane.shape
    p = plane[shave:h - shave, shave:w - shave]
    nh, nw = p.shape[0] // block, p.shape[1] // block
    return np.ascontiguousarray(p[:nh * block, :nw * block]), nh, nw


def mscn(plane):
    k = np.outer(window(), window())
    mu = ndimage.convolve(plane, k, mode='nearest')
    sigma = np.sqrt(np.abs(ndimage.convolve(plane * plane, k, mode='nearest') - mu * mu))
    return (plane - mu) / (sigma + 1.0), sigma


def _reflect(idx, n):
    idx = np.where(idx < 0, -idx - 1, idx)
    return np.where(idx >= n, 2 * n - 1 - idx, idx)


def shrink(plane):
    """MATLAB's antialiased bicubic at exactly 1/2: rows first, then columns."""
    h, w = plane.shape
    rows = _reflect(2 * np.arange(h // 2)[:, None] - 3 + np.arange(8)[None, :], h)      # [h/2, 8]
    v = np.einsum('ik,ikx->ix', np.broadcast_to(SHRINK, rows.shape), plane[rows])
    cols = _reflect(2 * np.arange(w // 2)[:, None] - 3 + np.arange(8)[None, :], w)      # [w/2, 8]
    return np.einsum('jk,ijk->ij', np.broadcast_to(SHRINK, cols.shape), v[:, cols])


def aggd(m):
    """(alpha, beta_l, beta_r) of one map; NaNs for an empty side or an all-zero map."""
    m = m.ravel()
    neg, pos = m[m < 0], m[m > 0]
    q = np.sum(m * m)
    if neg.size == 0 or pos.size == 0 or q == 0:
        return np.nan, np.nan, np.nan
    ls, rs = np.sqrt(np.sum(neg * neg) / neg.size), np.sqrt(np.sum(pos * pos) / pos.size)
    gh = ls / rs
    rhat = (np.sum(np.abs(m)) / m.size) ** 2 / (q / m.size)
    rn = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    j = int(np.argmin((R_GAM - rn) ** 2))
    alpha = GAM[j]
    scale = np.sqrt(special.gamma(1.0 / alpha) / special.gamma(3.0 / alpha))
    return alpha, ls * scale, rs * scale


def block_features(B):
    """The 18 features of one b x b block of MSCN values."""
    alpha, bl, br = aggd(B)
    f = [alpha, (bl + br) / 2.0]
    for shift in SHIFTS:
        alpha, bl, br = aggd(B * np.roll(B, shift, axis=(0, 1)))
        mean = (br - bl) * (special.gamma(2.0 / alpha) / special.gamma(1.0 / alpha)) if alpha == alpha else np.nan
        f += [alpha, mean, bl, br]
    return f


def features(img, shave=0, block=96, sharpness=False):
    """img: [C,H,W] float32 or uint8 numpy -> [blocks, 36] fp64 (and the per-block mean of scale 1's sigma)."""
    plane, nh, nw = crop(luma(quantise(np.asarray(img))), shave, block)
    assert nh * nw >= 2, (nh, nw)
    out = np.empty((nh * nw, 36))
    sharp = np.empty(nh * nw)
    for s, b in ((0, block), (1, block // 2)):
        n, sigma = mscn(plane)
        for by in range(nh):
            for bx in range(nw):
                sl = (slice(by * b, by * b + b), slice(bx * b, bx * b + b))
                out[by * nw + bx, 18 * s:18 * s + 18] = block_features(n[sl])
                if s == 0:
                    sharp[by * nw + bx] = sigma[sl].mean()
        if s == 0:
            plane = shrink(plane)
    return (out, sharp) if sharpness else out


def finish(F, mu_p, cov_p):
    good = F[~np.isnan(F).any(axis=1)]
    if good.shape[0] < 2:
        raise ValueError("fewer than 2 NaN-free rows")
    mu = np.nanmean(F, axis=0)
    cov = np.cov(good, rowvar=False)
    d = np.asarray(mu_p, dtype=np.float64).reshape(-1) - mu
    return float(np.sqrt(d @ np.linalg.pinv((np.asarray(cov_p) + cov) / 2.0) @ d))


def fit_params(pictures, block=96, sharp=0.75):
    """NIQE's own fit: per picture the blocks sharper than `sharp` times the picture's sharpest, NaN rows dropped."""
    rows = []
    for img in pictures:
        F, s = features(img, 0, block, sharpness=True)
        keep = (s > sharp * s.max()) & ~np.isnan(F).any(axis=1)
        rows.append(F[keep])
    rows = np.concatenate(rows)
    return rows.mean(axis=0), np.cov(rows, rowvar=False), rows.shape[0]


def picture(seed, c, h, w):
    """Seeded 8-bit picture [c,h,w]: Gaussian-filtered noise (sigma 1.2, scaled to a standard deviation of 60 grey levels)
    on a ramp."""
    rng = np.random.RandomState(seed)
    noise = ndimage.gaussian_filter(rng.randn(c, h, w), sigma=(0, 1.2, 1.2))
    noise *= 60.0 / noise.std()
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 128.0 + 50.0 * (xx / float(w) - 0.5) + 30.0 * (yy / float(h) - 0.5)
    return np.clip(np.rint(ramp[None] + noise), 0, 255).astype(np.uint8)


# name -> (seed, (c, h, w), block, shave, flat): `flat` = (y0, y1, x0, x1) set to the grey FLAT_GREY first, or None.
# A block is "made constant" by flattening it AND the 9 pixels around it that its scale-2 values reach (3 for the window
# at scale 1; 2 * 3 + 3 at scale 2), so its MSCN values are all zero at both scales and its 36 features are NaN.  Block
# (0, 0) is used: the plane's borders replicate the grey.  The grey is not arbitrary.  On a constant plane of level L the
# window returns L (1 + d) with d = 0 or a rounding of 1e-16, and NIQE counts the SIGN of P - mu: with d != 0 every flat
# pixel of the neighbouring blocks is counted as negative by one order of summation and as zero or positive by another,
# and no bar can hold two implementations together.  RGB 88 has luma 92, one of the levels (0, 23, 46, 92, 135, 184) at
# which scipy's 49-tap sum and the separable 7 + 7 sums are both exact (d = 0, checked by test_niqe_cpu.py).
FLAT_GREY = 88
CASES = {
    "2x2_exact":      (11, (3, 32, 32), 16, 0, None),
    "remainders_nan": (12, (3, 50, 70), 16, 0, (0, 25, 0, 25)),
    "grey_block8":    (13, (1, 40, 56), 8, 0, None),
    "block96":        (14, (3, 197, 99), 96, 0, None),
    "block24_shave3": (15, (3, 70, 50), 24, 3, None),
    "one_block_row":  (16, (1, 16, 130), 16, 0, None),
}
NAN_ROWS = {"remainders_nan": [0]}   # the blocks each case made constant (grid index by * nw + bx)


@functools.lru_cache(maxsize=None)
def case_picture(name):
    seed, (c, h, w), block, shave, flat = CASES[name]
    img = picture(seed, c, h, w)
    if flat:
        img[:, flat[0]:flat[1], flat[2]:flat[3]] = FLAT_GREY
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(features [blocks, 36], sharpness [blocks]) of a case by the restatement: computed once, shared, read-only."""
    _, _, block, shave, _ = CASES[name]
    F, s = features(case_picture(name), shave, block, sharpness=True)
    F.setflags(write=False), s.setflags(write=False)
    return F, s


@functools.lru_cache(maxsize=None)
def fitted_params():
    """mu_p, cov_p fitted by the restatement from eight seeded [3, 64, 80] pictures at block 16."""
    mu, cov, rows = fit_params([picture(100 + i, 3, 64, 80) for i in range(8)], block=16)
    mu.setflags(write=False), cov.setflags(write=False)
    return mu, cov, rows


def assert_features(got, want, what=""):
    """The feature bar: identical NaN positions, |got - want| <= FEATURE_TOL * max(1, |want|) on every other element.
    Returns the worst ratio |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all(), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:8])
    ok = ~np.isnan(want)
    ratio = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%-40s worst |dev - ref| / max(1, |ref|) = %.3e" % (what, worst))
    assert worst <= FEATURE_TOL, (what, worst)
    return worst
