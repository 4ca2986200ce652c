"""The yardstick of the motion-compensation operators: warp, motion_fuse and flow_huber restated in numpy
float64, in pixel coordinates with no normalisation, with their flow gradients written out; and the case table the CPU and
GPU tests share.

warp(img [N,C,H,W], flow [N,2,H,W]): flow channel 0 is the x displacement, channel 1 the y displacement, in pixels.
  xs = x + flow_x, ys = y + flow_y, clamped to [0, W-1] / [0, H-1]; x0 = floor(xs), x1 = min(x0 + 1, W-1), wx = xs - x0,
  the same in y; the bilinear value.  d/dflow_x = ((v01 - v00)(1 - wy) + (v11 - v10) wy) * [0 < unclamped xs < W-1],
  symmetric in y: on an integer coordinate the right-hand cell's slope.
  This is F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True); torch's normalise / un-normalise
  round trip can land below an integer coordinate and take the left cell, so torch is a cross-check on the off-integer
  family only (tests/test_mc_cpu.py).
motion_fuse(frames [N,3,C,H,W], flow [2N,2,H,W]): fused = [warp(t-1, flow[:N]) | frame t | warp(t+1, flow[N:])],
  mc = mean over all 2 N C H W elements of (warped - frame t)^2.
flow_huber(flow [M,2,H,W], eps): forward differences of both components, 0 at the last column and row;
  h = sqrt(eps + dx_u^2 + dy_u^2 + dx_v^2 + dy_v^2) per pixel; the mean over M H W.
"""
import numpy as np

# (N, C, H, W)
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 5), (2, 3, 5, 1), (1, 1, 4, 4), (2, 3, 7, 9), (1, 1, 17, 70), (3, 3, 32, 32)]
FAMILIES = ("odd128", "quarter")


def _taps(flow):
    f = np.asarray(flow, dtype=np.float64)
    n, _, h, w = f.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ux, uy = xs[None] + f[:, 0], ys[None] + f[:, 1]                  # unclamped
    mx = ((ux > 0) & (ux < w - 1)).astype(np.float64)
    my = ((uy > 0) & (uy < h - 1)).astype(np.float64)
    cx, cy = np.clip(ux, 0, w - 1), np.clip(uy, 0, h - 1)
    x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    return dict(ux=ux, uy=uy, x0=x0, x1=x1, y0=y0, y1=y1, wx=cx - x0, wy=cy - y0, mx=mx, my=my)


def coordinates(flow):
    """The unclamped sample coordinates (ux, uy), each [N,H,W] float64."""
    t = _taps(flow)
    return t["ux"], t["uy"]


def warp(img, flow, g=None):
    """-> (out [N,C,H,W], dflow [N,2,H,W]) in float64; dflow = d sum(g * out) / d flow (g None: zeros)."""
    img = np.asarray(img, dtype=np.float64)
    n, c, h, w = img.shape
    t = _taps(flow)
    b = np.arange(n)[:, None, None]
    out = np.empty((n, c, h, w))
    dflow = np.zeros((n, 2, h, w))
    for k in range(c):
        p = img[:, k]
        v00, v01 = p[b, t["y0"], t["x0"]], p[b, t["y0"], t["x1"]]
        v10, v11 = p[b, t["y1"], t["x0"]], p[b, t["y1"], t["x1"]]
        wx, wy = t["wx"], t["wy"]
        out[:, k] = (v00 * (1 - wx) + v01 * wx) * (1 - wy) + (v10 * (1 - wx) + v11 * wx) * wy
        if g is not None:
            gk = np.asarray(g, dtype=np.float64)[:, k]
            dflow[:, 0] += gk * ((v01 - v00) * (1 - wy) + (v11 - v10) * wy) * t["mx"]
            dflow[:, 1] += gk * ((v10 - v00) * (1 - wx) + (v11 - v01) * wx) * t["my"]
    return out, dflow


def motion_fuse(frames, flow, g_fused=None, seed=1.0):
    """-> (fused [N,3C,H,W], mc, dflow [2N,2,H,W]); dflow = d (sum(g_fused * fused) + seed * mc) / d flow."""
    frames = np.asarray(frames, dtype=np.float64)
    n, _, c, h, w = frames.shape
    cur = frames[:, 1]
    numel = 2 * n * c * h * w
    fused = np.empty((n, 3 * c, h, w))
    fused[:, c:2 * c] = cur
    dflow = np.empty((2 * n, 2, h, w))
    sq = 0.0
    for k, (src, lo) in enumerate(((frames[:, 0], 0), (frames[:, 2], 2 * c))):
        fl = np.asarray(flow)[k * n:(k + 1) * n]
        warped, _ = warp(src, fl)
        fused[:, lo:lo + c] = warped
        sq += ((warped - cur) ** 2).sum()
        up = seed * 2.0 / numel * (warped - cur)
        if g_fused is not None:
            up = up + np.asarray(g_fused, dtype=np.float64)[:, lo:lo + c]
        dflow[k * n:(k + 1) * n] = warp(src, fl, up)[1]
    return fused, sq / numel, dflow


def flow_huber(flow, eps=0.01, grad_scale=1.0):
    """-> (loss, grad_scale * d loss / d flow [M,2,H,W]) in float64."""
    f = np.asarray(flow, dtype=np.float64)
    m, _, h, w = f.shape
    dx, dy = np.zeros_like(f), np.zeros_like(f)
    dx[..., :-1] = f[..., 1:] - f[..., :-1]
    dy[..., :-1, :] = f[..., 1:, :] - f[..., :-1, :]
    hub = np.sqrt(eps + (dx ** 2).sum(1) + (dy ** 2).sum(1))            # [M,H,W]
    ax, ay = dx / hub[:, None], dy / hub[:, None]                       # d h(p) / d dx(p), d h(p) / d dy(p)
    g = -(ax + ay)
    g[..., 1:] += ax[..., :-1]
    g[..., 1:, :] += ay[..., :-1, :]
    return hub.mean(), grad_scale * g / (m * h * w)


def flows(family, rows, h, w, seed):
    """The table's flows [rows,2,H,W] float32, exact in fp32 together with the pixel index.
    odd128: odd multiples of 1/128 in +-3 px (+-1 on a side under 8): never nearer than 1/128 to an integer.
    quarter: multiples of 1/4 in the same range: they land on integers and on the clamp bounds."""
    rng = np.random.RandomState(seed)
    out = np.empty((rows, 2, h, w), dtype=np.float32)
    for ch, side in ((0, w), (1, h)):
        r = 3 if side >= 8 else 1
        if family == "odd128":
            k = rng.randint(-64 * r, 64 * r, size=(rows, h, w)) * 2 + 1       # odd, |k| <= 128 r - 1
            out[:, ch] = k / 128.0
        elif family == "quarter":
            out[:, ch] = rng.randint(-4 * r, 4 * r + 1, size=(rows, h, w)) / 4.0
        else:
            raise ValueError(family)
    return out


def case(shape, family, seed=0):
    """frames [N,3,C,H,W] float32 in [0, 1) and flow [2N,2,H,W] float32 of one table row."""
    n, c, h, w = shape
    rng = np.random.RandomState(1000 + seed + 7 * n + 31 * c + 101 * h + 1009 * w)
    frames = rng.rand(n, 3, c, h, w).astype(np.float32)
    return frames, flows(family, 2 * n, h, w, seed + 17 * h + w)


def cases():
    return [(s, f) for s in SHAPES for f in FAMILIES]


def bar_out(ref):
    """The project's contract for outputs and losses: 1e-4 max|ref| (+ 1e-9 where the reference can be 0)."""
    return 1e-4 * float(np.max(np.abs(ref))) + 1e-9


def bar_grad(ref):
    return 1e-3 * float(np.max(np.abs(ref))) + 1e-9
