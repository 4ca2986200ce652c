"""The streaming kernels (csrc/elementwise.hip, loss_optim.hip, prepost.hip) as their formulas read, in numpy float64,
for the tests -- plus the inputs both test files (test_streaming_cpu / test_streaming_gpu) feed them.

Conventions
  * arrays arrive in MEMORY order: an activation of C channels is [..., C] (dense NHWC, or [B, F]); nothing here calls
    the op under test.
  * every function takes `dt`: float64 is the reference, float32 the same formula in the arithmetic the kernels have
    (test_streaming_cpu measures that against the reference to show what a bar leaves).
  * hyper-parameters are what the C ABI carries: fp32 values.  `f32(v)` is the double that equals float(v) -- 0.999
    is 0.99900001287 on the device, and a reference fed the double 0.999 would differ by 1.3e-5 in Adam's second moment
    for no fault of a kernel.
  * a backward takes the tensor the kernel reads: the saved OUTPUT for relu / lrelu / tanh / sigmoid, the input for PReLU.
"""
import numpy as np

BAR = 1e-6            # element-wise (conftest.assert_close_elementwise) and relative (scalar reductions)
BAR_DPRELU = 1e-5     # PReLU slope gradient: float atomics in arbitrary order (test_ops_gpu.test_activation)
ACTS = ("relu", "prelu", "prelu_c", "lrelu", "tanh", "sigmoid")
ACT_CODE = {"relu": 1, "prelu": 2, "prelu_c": 2, "lrelu": 3, "tanh": 4, "sigmoid": 5}
LOSSES = ("mse", "l1", "charbonnier", "bce")


def f32(v):
    return float(np.float32(v))


def frac_of_bar(got, ref, rtol=BAR, atol=None):
    """max |got - ref| / (atol + rtol |ref|): the share of assert_close_elementwise's allowance that is used (same default
    atol = rtol * rms(ref))."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if atol is None:
        atol = rtol * float(np.sqrt(np.mean(ref * ref))) if ref.size else 0.0
    den = atol + rtol * np.abs(ref)
    diff = np.abs(got - ref)
    return float(np.max(np.where(diff == 0, 0.0, diff / np.where(den == 0, 1e-300, den))))


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
def act_fwd(x, kind, slope=0.0, w=None, dt=np.float64):
    """x [..., C]; w: None, [1] or [C].  Zero (either sign) takes the slope side of prelu / lrelu."""
    x = np.asarray(x, dt)
    if kind == "relu":
        return np.where(x > 0, x, dt(0))
    if kind == "lrelu":
        return np.where(x > 0, x, x * dt(slope))
    if kind in ("prelu", "prelu_c"):
        return np.where(x > 0, x, x * np.asarray(w, dt))
    if kind == "tanh":
        return np.tanh(x)
    if kind == "sigmoid":
        return dt(1) / (dt(1) + np.exp(-x))
    raise ValueError(kind)


def act_bwd(dy, saved, kind, slope=0.0, w=None, dt=np.float64):
    """-> (dx, dw or None).  saved = y for relu / lrelu / tanh / sigmoid, x for prelu.  torch's conventions at zero:
    relu' = 0, prelu / lrelu take the slope; the slope gradient there is dy * 0."""
    g, s = np.asarray(dy, dt), np.asarray(saved, dt)
    if kind == "relu":
        return np.where(s > 0, g, dt(0)), None
    if kind == "lrelu":
        return np.where(s > 0, g, g * dt(slope)), None
    if kind in ("prelu", "prelu_c"):
        w = np.asarray(w, dt)
        dx = np.where(s > 0, g, g * w)
        dsl = np.where(s > 0, dt(0), g * s)
        dw = dsl.reshape(-1, w.size).sum(axis=0) if w.size > 1 else dsl.sum().reshape(1)
        return dx, dw
    if kind == "tanh":
        return g * (dt(1) - s * s), None
    if kind == "sigmoid":
        return g * s * (dt(1) - s), None
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------
# losses (mean reduction): value and d value / d pred
# ------------------------------------------------------------------------------------------------
def loss(kind, p, t, eps=0.0, dt=np.float64):
    p, t = np.asarray(p, dt), np.asarray(t, dt)
    n = p.size
    d = p - t
    if kind == "mse":
        val, g = d * d, dt(2) * d
    elif kind == "l1":
        val, g = np.abs(d), np.sign(d)
    elif kind == "charbonnier":
        e = np.sqrt(d * d + dt(eps))
        val, g = e, d / e
    elif kind == "bce":   # torch: logs clamped at -100, the gradient's denominator at 1e-12
        with np.errstate(divide="ignore"):
            lp = np.maximum(np.log(p), dt(-100))
            l1p = np.maximum(np.log(dt(1) - p), dt(-100))
        val = -(t * lp + (dt(1) - t) * l1p)
        g = d / np.maximum((dt(1) - p) * p, dt(f32(1e-12)))
    else:
        raise ValueError(kind)
    # (the mean itself in float64 for either dt: the kernels sum block partials in double)
    return float(np.sum(val, dtype=np.float64) / n), (g / dt(n)).astype(dt)


# ------------------------------------------------------------------------------------------------
# optimizers and the norm clip
# ------------------------------------------------------------------------------------------------
def sgd_step(p, g, buf, lr, mom=0.0, wd=0.0, nesterov=False, first=False, gs=1.0, dt=np.float64):
    """torch.optim.SGD with dampening 0 -> (p, buf).  first: the buffer is not read (torch's buf = clone(d))."""
    p, g = np.asarray(p, dt), np.asarray(g, dt)
    d = g * dt(gs)
    if wd != 0:
        d = d + dt(wd) * p
    if mom != 0:
        buf = d.copy() if first else np.asarray(buf, dt) * dt(mom) + d
        d = d + dt(mom) * buf if nesterov else buf
    return p - dt(lr) * d, buf


def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd=0.0, gs=1.0, dt=np.float64):
    """torch/optim/adam.py _single_tensor_adam without amsgrad; `step` counts the steps BEFORE this one.
    -> (p, m, v, step + 1).  The bias corrections are Python doubles there, for either dt."""
    p, g, m, v = (np.asarray(a, dt) for a in (p, g, m, v))
    t = step + 1
    g = g * dt(gs)
    if wd != 0:
        g = g + dt(wd) * p
    m = m + (g - m) * dt(1.0 - b1)                       # exp_avg.lerp_(grad, 1 - beta1)
    v = v * dt(b2) + dt(1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = np.sqrt(v) / dt(bc2 ** 0.5) + dt(eps)
    return p - dt(lr / bc1) * (m / denom), m, v, t


def clip(g, max_norm):
    """torch.nn.utils.clip_grad_norm_ -> (norm, scale)."""
    g = np.asarray(g, np.float64)
    norm = float(np.sqrt(np.sum(g * g)))
    return norm, min(1.0, max_norm / (norm + 1e-6))


# ------------------------------------------------------------------------------------------------
# the rest
# ------------------------------------------------------------------------------------------------
def absmax(x):
    return float(np.max(np.abs(np.asarray(x, np.float64))))


def psnr(pred, gt):
    """utils.PSNR: clamp and difference in fp32, mean in float64 -> (psnr, mse)."""
    d = np.clip(np.asarray(pred, np.float32), np.float32(0), np.float32(1)) - np.asarray(gt, np.float32)
    mse = float(np.mean(d.astype(np.float64) ** 2))
    return (100.0 if mse == 0 else 10.0 * np.log10(1.0 / mse)), mse


def channel_affine(x, sub, div, clamp01=False, dt=np.float64):
    """x [N, C, H, W] (logical)."""
    x = np.asarray(x, dt)
    c = x.shape[1]
    y = (x - np.asarray(sub[:c], dt).reshape(1, c, 1, 1)) / np.asarray(div[:c], dt).reshape(1, c, 1, 1)
    return np.clip(y, dt(0), dt(1)) if clamp01 else y


def upsample_fwd(x, r):
    """x [N, C, H, W] -> [N, C, H r, W r], y[.., oy, ox] = x[.., oy // r, ox // r]."""
    return np.repeat(np.repeat(np.asarray(x), r, axis=2), r, axis=3)


def upsample_bwd(dy, r):
    dy = np.asarray(dy, np.float64)
    n, c, hr, wr = dy.shape
    return dy.reshape(n, c, hr // r, r, wr // r, r).sum(axis=(3, 5))


def maxpool2(x):
    """2x2, stride 2, floor mode: an odd trailing row / column is dropped."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    v = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2)
    return v.max(axis=(3, 5))


# ------------------------------------------------------------------------------------------------
# launch geometry, as the launchers of the three files compute it (blocks of 256 threads, grid-stride loops)
# ------------------------------------------------------------------------------------------------
def _blocks(items, per_block, cap):
    return max(1, min(cap, (items + per_block - 1) // per_block))


SMALL = (1, 2, 3, 4, 5, 7, 8, 1020, 1023, 1024, 1025, 1028, 4096, 4099, 6145)
CAP_EW = 4096 * 2048          # grid_for(n, 256 * 8, 4096): act forward / scalar backward / axpby; k_act_bwd<4>: (n / 4, 512, 4096)
CAP_RED = 1024 * 2048         # grid_for(n, 256 * 8, 1024): scalar loss / sgd / adam / grad norm; psnr (4096, then kPsnrPartials)
CAP_LOSS4 = 4 * 1024 * 256    # k_loss_partial<4>: one float4 per thread and pass, kMaxPartials blocks
CAP_ADAM4 = 4 * 512 * 512     # k_adam<4>: two float4 per thread, 2 * CUs blocks (256 CUs)
CAP_ABSMAX = 1024 * 4096
CAP_PP = 4096 * 1024          # grid_for(n, 256 * 4, 4096): channel_affine, maxpool, scalar up-sample
CAP_UP4 = 4 * 4096 * 512      # float4 up-sample: grid_for(total / 4, 256 * 2, 4096)
# (k_sgd<4>'s cap of 65535 blocks of 512 float4 needs > 500 MB per buffer: not swept)


def sizes(cap, cap2=None):
    """The structural sizes of one family: SMALL, then just above the cap with n % 4 == 3 and its multiple-of-4 neighbour."""
    out = list(SMALL) + [cap + 3, cap + 4]
    if cap2:
        out += [cap2 + 3, cap2 + 4]
    return out


def grid_red(n):
    return _blocks(n, 2048, 1024)


def grid_loss(n, vec):
    return _blocks(n // 4, 256, 1024) if vec else grid_red(n)


def grid_absmax(n):
    return _blocks(n, 4096, 1024)


def positions(n, blocks, width=1):
    """Where a streaming reduction over n elements with `blocks` blocks of 256 threads reading `width` elements each
    can lose or repeat one: the last element, the last element of the float4 body, the first element of the second
    grid-stride pass, the first element of the last block.  Sorted, unique, inside [0, n)."""
    cand = (n - 1, n // 4 * 4 - 1, blocks * 256 * width, (blocks - 1) * 256 * width)
    return sorted(set(i for i in cand if 0 <= i < n))


# ------------------------------------------------------------------------------------------------
# inputs (numpy MT19937: platform independent), shared by the CPU and the GPU file
# ------------------------------------------------------------------------------------------------
def _rs(seed):
    return np.random.RandomState(seed)


def gen_act(n, seed=3):
    """(x, dy): N(0, 2^2) with exact +0.0 / -0.0 sprinkled in."""
    rs = _rs(seed)
    x = (rs.standard_normal(n) * 2).astype(np.float32)
    x[::7] = 0.0
    x[3::11] = -0.0
    return x, rs.standard_normal(n).astype(np.float32)


def gen_prelu_w(c, seed=5):
    """slopes of both signs"""
    return (0.25 * _rs(seed).standard_normal(c) + 0.1).astype(np.float32) * np.where(np.arange(c) % 2, -1, 1).astype(np.float32)


def gen_loss(kind, n, where=(), seed=11):
    """(pred, target) flat.  |pred - target| ~ 1e-3, and 1000 x that at the indices `where` (planted mass: dropping or
    repeating one of them moves the mean by far more than the bar).  BCE: hard labels, pred 1e-3 off the label, and
    e^-20 off the WRONG label where planted (a term of 20 against 1e-3)."""
    rs = _rs(seed)
    where = np.asarray(where, np.int64)
    if kind == "bce":
        t = (rs.uniform(size=n) < 0.5).astype(np.float32)
        off = (1e-3 * (0.5 + rs.uniform(size=n))).astype(np.float32)
        p = np.where(t > 0, np.float32(1) - off, off).astype(np.float32)
        p[where] = np.where(t[where] > 0, np.float32(np.exp(-20.0)), np.float32(1) - np.float32(2.0 ** -24 * 35))
        return p, t
    t = rs.uniform(size=n).astype(np.float32)
    p = (t + 1e-3 * rs.standard_normal(n)).astype(np.float32)
    p[where] = t[where] + np.where(np.arange(where.size) % 2, -1, 1).astype(np.float32)
    return p, t


def gen_mass(n, where=(), seed=13):
    """A gradient / difference vector ~ 1e-3 N(0,1) with +-1 planted at `where`."""
    g = (1e-3 * _rs(seed).standard_normal(n)).astype(np.float32)
    where = np.asarray(where, np.int64)
    g[where] = np.where(np.arange(where.size) % 2, -1, 1).astype(np.float32)
    return g


def gen_opt(n, steps=3, seed=17):
    """(p0, [g_1 .. g_steps]): 0.5 <= |p0| < 1.5; gradients N(0,1) with exact zeros and +-1e-12 (Adam's eps-dominated
    denominator) at fixed places in every step.  No denormals."""
    rs = _rs(seed)
    p0 = ((0.5 + rs.uniform(size=n)) * np.where(rs.uniform(size=n) < 0.5, -1, 1)).astype(np.float32)
    gs = []
    for _ in range(steps):
        g = rs.standard_normal(n).astype(np.float32)
        g[::5] = 0.0
        g[1::10] = 1e-12
        g[6::10] = -1e-12
        gs.append(g)
    return p0, gs


ADAM = dict(lr=f32(0.05), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))   # three steps move p by ~0.15: 0.1 .. 0.3 of |p|
SGD_VARIANTS = {"plain": dict(mom=0.0, wd=0.0, nesterov=False),
                "momentum": dict(mom=f32(0.9), wd=0.0, nesterov=False),
                "momentum_wd": dict(mom=f32(0.9), wd=f32(1e-4), nesterov=False),
                "nesterov": dict(mom=f32(0.9), wd=0.0, nesterov=True)}
SGD_LR = f32(0.05)


def run_sgd(p0, grads, variant, gs=1.0, dt=np.float64):
    """the chained steps -> (p, buf)"""
    p, buf = np.asarray(p0, dt), None
    for k, g in enumerate(grads):
        p, buf = sgd_step(p, g, buf, SGD_LR, first=(k == 0), gs=gs, dt=dt, **SGD_VARIANTS[variant])
    return p, buf


def run_adam(p0, grads, wd=0.0, gs=1.0, dt=np.float64):
    p = np.asarray(p0, dt)
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    for g in grads:
        p, m, v, t = adam_step(p, g, m, v, t, wd=wd, gs=gs, dt=dt, **ADAM)
    return p, m, v, t
