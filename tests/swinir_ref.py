"""fp64 plain-torch restatement of shifted-window attention and of SwinIR (Liang et al., ICCVW 2021; Liu et al., ICCV
2021), written from the papers' definition: roll, window partition, a gathered relative-position bias, the -100 mask of
the shifted configuration, softmax.  Nothing here touches the package's kernels; the tests hold the kernels, the host twin
and the net to it."""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

# N, H, W, C, heads, window, shift: the smallest shapes at which each index path can go wrong
CASES = {
    "one_window": (1, 4, 4, 4, 1, 4, 0),
    "2x3_windows": (2, 8, 12, 8, 2, 4, 2),       # H != W, every mask class, the roll wraps in both axes
    "9_tokens": (1, 6, 9, 6, 2, 3, 1),           # lanes idle, odd window
    "d30_classical": (2, 16, 16, 60, 2, 8, 4),
    "d10_lightweight": (1, 16, 24, 60, 6, 8, 4),
    "d32_shift3": (1, 16, 16, 64, 2, 8, 3),      # the register ceiling, a shift that is not half the window
    "4_tokens": (3, 8, 8, 16, 4, 2, 1),
    # beyond the issue's table: the any-window kernels at the two larger head-dimension classes (window 8 has kernels of
    # its own, and every case above with another window has d <= 8)
    "d12_window4": (1, 4, 8, 24, 2, 4, 1),
    "d32_window4": (2, 8, 4, 32, 1, 4, 2),
}


def worst(got, want):
    """max |got - want| relative to max |want| (the project's bar is stated this way)."""
    want = want.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def inputs(case, seed=0):
    """(qkv [N,H,W,3C], table [(2w-1)^2, heads], dout [N,H,W,C]) in fp32."""
    n, h, w, c, heads, window, shift = case
    return (rand((n, h, w, 3 * c), seed + 1, 1.5), rand(((2 * window - 1) ** 2, heads), seed + 2, 2.0),
            rand((n, h, w, c), seed + 3))


def rel_index(window):
    """[T, T] rows of the bias table: (y_i - y_j + w - 1) * (2w - 1) + (x_i - x_j + w - 1)."""
    ys, xs = torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")
    coords = torch.stack([ys.flatten(), xs.flatten()])                 # 2, T
    rel = coords[:, :, None] - coords[:, None, :] + (window - 1)       # 2, T, T
    return rel[0] * (2 * window - 1) + rel[1]


def region_image(h, w, window, shift):
    """[H, W] region ids of the SHIFTED map: three slices per axis, numbered row-major."""
    img = torch.zeros(h, w, dtype=torch.int64)
    cnt = 0
    for hs in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
        for ws in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
            img[hs, ws] = cnt
            cnt += 1
    return img


def partition(x, window):
    """[N, H, W, C] -> [N * windows, T, C], windows row-major."""
    n, h, w, c = x.shape
    x = x.view(n, h // window, window, w // window, window, c)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, window * window, c)


def reverse(wins, window, n, h, w):
    c = wins.shape[-1]
    x = wins.view(n, h // window, w // window, window, window, c)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)


def mask_tensor(h, w, window, shift):
    """[windows, T, T]: -100 where the two tokens' regions differ, else 0 (zeros without a shift)."""
    nwin, t = (h // window) * (w // window), window * window
    if shift == 0:
        return torch.zeros(nwin, t, t, dtype=torch.float64)
    ids = partition(region_image(h, w, window, shift)[None, :, :, None], window)[:, :, 0]     # windows, T
    return torch.where(ids[:, :, None] != ids[:, None, :], -100.0, 0.0).double()


def window_attention(qkv, table, heads, window, shift, masked=True):
    """The operator on [N, H, W, 3C] (any float dtype; computed in it)."""
    n, h, w, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    wins = partition(x, window)                                        # B, T, 3C
    b, t, _ = wins.shape
    q, k, v = wins.view(b, t, 3, heads, d).permute(2, 0, 3, 1, 4)      # each B, heads, T, d
    s = (q * d ** -0.5) @ k.transpose(-2, -1)
    bias = table[rel_index(window).flatten()].view(t, t, heads).permute(2, 0, 1)
    s = s + bias[None].to(s.dtype)
    if shift and masked:
        m = mask_tensor(h, w, window, shift).to(s.dtype)
        s = (s.view(n, -1, heads, t, t) + m[None, :, None]).view(b, heads, t, t)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, t, c)
    o = reverse(o, window, n, h, w)
    return torch.roll(o, (shift, shift), (1, 2)) if shift else o


def attention_with_grads(case, seed=0):
    """(out, dqkv, dtable) in fp64 from autograd of the restatement."""
    n, h, w, c, heads, window, shift = case
    qkv, table, dout = inputs(case, seed)
    q64, t64 = qkv.double().requires_grad_(), table.double().requires_grad_()
    out = window_attention(q64, t64, heads, window, shift)
    out.backward(dout.double())
    return out.detach(), q64.grad, t64.grad


class Host(object):
    pass


def host(lib, case, seed=0, backward=True):
    """srk_window_attention_host on the same inputs."""
    n, h, w, c, heads, window, shift = case
    qkv, table, dout = (t.contiguous() for t in inputs(case, seed))
    r = Host()
    r.out = torch.zeros(n, h, w, c, dtype=torch.float64)
    r.dqkv = torch.zeros(n, h, w, 3 * c, dtype=torch.float64)
    r.dtable = torch.zeros_like(table, dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.srk_window_attention_host(p(qkv), p(table), p(dout) if backward else None, n, h, w, c, heads, window, shift,
                                       p(r.out), p(r.dqkv) if backward else None, p(r.dtable) if backward else None)
    assert rc == 0, lib.srk_last_error_string()
    return r


# ---- the net --------------------------------------------------------------------------------------------------------
class RefAttention(nn.Module):
    def __init__(self, dim, heads, window):
        super().__init__()
        self.heads, self.window = heads, window
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, shift):      # x: N, H, W, C
        return self.proj(window_attention(self.qkv(x), self.relative_position_bias_table, self.heads, self.window, shift))


class RefMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(dim, hidden), nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class RefLayer(nn.Module):
    def __init__(self, dim, heads, window, shift, mlp_ratio):
        super().__init__()
        self.shift = shift
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.attn = RefAttention(dim, heads, window)
        self.mlp = RefMlp(dim, int(dim * mlp_ratio))

    def forward(self, x):
        x = x + self.attn(self.norm1(x), self.shift)
        return x + self.mlp(self.norm2(x))


class RefGroup(nn.Module):
    def __init__(self, dim, depth, heads, window, mlp_ratio):
        super().__init__()
        self.blocks = nn.ModuleList([RefLayer(dim, heads, window, 0 if j % 2 == 0 else window // 2, mlp_ratio)
                                     for j in range(depth)])


class RefRSTB(nn.Module):
    def __init__(self, dim, depth, heads, window, mlp_ratio):
        super().__init__()
        self.residual_group = RefGroup(dim, depth, heads, window, mlp_ratio)
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1)

    def forward(self, x):             # N, H, W, C
        y = x
        for blk in self.residual_group.blocks:
            y = blk(y)
        return self.conv(y.permute(0, 3, 1, 2)).permute(0, 2, 3, 1) + x


class RefNorm(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim)


RGB_MEAN = (0.4488, 0.4371, 0.4040)


class RefSwinIR(nn.Module):
    def __init__(self, num_channels, embed_dim, depths, num_heads, window_size, mlp_ratio, scale_factor, upsampler):
        super().__init__()
        self.window, self.scale, self.upsampler = window_size, scale_factor, upsampler
        mean = torch.tensor(RGB_MEAN if num_channels == 3 else (0.0,) * num_channels, dtype=torch.float64)
        self.register_buffer("mean", mean.view(1, -1, 1, 1), persistent=False)
        self.conv_first = nn.Conv2d(num_channels, embed_dim, 3, 1, 1)
        self.patch_embed = RefNorm(embed_dim)
        self.layers = nn.ModuleList([RefRSTB(embed_dim, d, num_heads, window_size, mlp_ratio) for d in depths])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        if upsampler == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, 64, 3, 1, 1), nn.LeakyReLU(inplace=True))
            up = []
            if scale_factor == 3:
                up = [nn.Conv2d(64, 9 * 64, 3, 1, 1), nn.PixelShuffle(3)]
            else:
                for _ in range(int(math.log2(scale_factor))):
                    up += [nn.Conv2d(64, 4 * 64, 3, 1, 1), nn.PixelShuffle(2)]
            self.upsample = nn.Sequential(*up)
            self.conv_last = nn.Conv2d(64, num_channels, 3, 1, 1)
        else:
            self.upsample = nn.Sequential(nn.Conv2d(embed_dim, scale_factor ** 2 * num_channels, 3, 1, 1),
                                          nn.PixelShuffle(scale_factor))

    def forward(self, x):
        h, w = x.shape[2:]
        ph, pw = (-h) % self.window, (-w) % self.window
        if ph or pw:                  # reflect padding at the bottom and the right
            x = F.pad(x, (0, pw, 0, ph), mode="reflect")
        x = x - self.mean
        first = self.conv_first(x)
        t = self.patch_embed.norm(first.permute(0, 2, 3, 1))
        for layer in self.layers:
            t = layer(t)
        body = self.conv_after_body(self.norm(t).permute(0, 3, 1, 2)) + first
        if self.upsampler == "pixelshuffle":
            out = self.conv_last(self.upsample(self.conv_before_upsample(body)))
        else:
            out = self.upsample(body)
        out = out + self.mean
        return out[:, :, :h * self.scale, :w * self.scale]


def ref_swinir_like(net, *ctor):
    """The fp64 plain net with the package net's parameters."""
    ref = RefSwinIR(*ctor).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in net.state_dict().items()})
    return ref
