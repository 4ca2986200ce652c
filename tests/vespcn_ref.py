"""VESPCN restated in torch (any dtype, float64 for the yardstick) from a models.VESPCNNet state_dict: the net, its three
loss terms and the training loss.  The warp is written in pixel coordinates with its clamp masks written out, so autograd
gives the stated one-sided convention of tests/mc_ref.py (the gradient by a flow component is the bilinear slope where the
unclamped coordinate lies strictly inside the picture, else 0)."""
import torch
import torch.nn.functional as F


def warp(img, flow):
    """img [N,C,H,W], flow [N,2,H,W] in pixels (x then y) -> the bilinear samples at (x + flow_x, y + flow_y), clamped."""
    n, c, h, w = img.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=img.dtype), torch.arange(w, dtype=img.dtype), indexing="ij")

    def axis(base, f, side):
        u = base[None] + f                                  # unclamped, carries the gradient
        m = ((u > 0) & (u < side - 1)).to(img.dtype).detach()
        cs = u.detach().clamp(0, side - 1)
        i0 = cs.floor()
        wgt = (cs - i0) + m * (u - u.detach())              # the value of cs - i0, the gradient m
        i0 = i0.long()
        return i0, (i0 + 1).clamp(max=side - 1), wgt

    x0, x1, wx = axis(xs, flow[:, 0], w)
    y0, y1, wy = axis(ys, flow[:, 1], h)
    flat = img.reshape(n, c, h * w)

    def at(yy, xx):
        return flat.gather(2, (yy * w + xx).reshape(n, 1, h * w).expand(n, c, h * w)).reshape(n, c, h, w)

    wx, wy = wx[:, None], wy[:, None]
    return (at(y0, x0) * (1 - wx) + at(y0, x1) * wx) * (1 - wy) + (at(y1, x0) * (1 - wx) + at(y1, x1) * wx) * wy


def coordinates(flow):
    """The unclamped sample coordinates of a flow [M,2,H,W]: (x + flow_x, y + flow_y)."""
    m, _, h, w = flow.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=flow.dtype), torch.arange(w, dtype=flow.dtype), indexing="ij")
    return xs[None] + flow[:, 0], ys[None] + flow[:, 1]


def flow_huber(flow, eps=0.01):
    dx = F.pad(flow[..., 1:] - flow[..., :-1], (0, 1))
    dy = F.pad(flow[..., 1:, :] - flow[..., :-1, :], (0, 0, 0, 1))
    return torch.sqrt(eps + (dx ** 2).sum(1) + (dy ** 2).sum(1)).mean()


def _stack(sd, prefix, x, specs, r):
    for i, (stride, pad) in enumerate(specs):
        x = F.conv2d(x, sd["%s.%d.conv.weight" % (prefix, i)], sd["%s.%d.conv.bias" % (prefix, i)], stride=stride, padding=pad)
        x = torch.relu(x) if i + 1 < len(specs) else x
    return F.pixel_shuffle(x, r)


def motion_flow(sd, pair, max_flow):
    """MotionCompensator: pair [M,2C,H,W] = [cur | nbr] -> (flow in pixels, coarse stage's flow in pixels)."""
    c = pair.shape[1] // 2
    coarse = torch.tanh(_stack(sd, "mc.coarse", pair, [(2, 2), (1, 1), (2, 2), (1, 1), (1, 1)], 4))
    warped = warp(pair[:, c:], max_flow * coarse)
    fine = torch.tanh(_stack(sd, "mc.fine", torch.cat([pair, coarse, warped], 1), [(2, 2), (1, 1), (1, 1), (1, 1), (1, 1)], 2))
    return max_flow * coarse + max_flow / 4.0 * fine, max_flow * coarse


def forward_terms(sd, frames, scale, max_flow=8.0):
    """frames [N,3,C,H,W] (H, W multiples of 4) -> (sr [N,C,r(H-8),r(W-8)], mc, flow [2N,2,H,W], coarse flow)."""
    n, _, c, h, w = frames.shape
    prev, cur, nxt = frames[:, 0], frames[:, 1], frames[:, 2]
    pair = torch.cat([torch.cat([cur, prev], 1), torch.cat([cur, nxt], 1)], 0)
    flow, coarse = motion_flow(sd, pair, max_flow)
    wa, wb = warp(prev, flow[:n]), warp(nxt, flow[n:])
    mc = (((wa - cur) ** 2).sum() + ((wb - cur) ** 2).sum()) / (2 * n * c * h * w)
    sr = _stack(sd, "layers", torch.cat([wa, cur, wb], 1), [(1, 0), (1, 0), (1, 0)], scale)
    return sr, mc, flow, coarse


def pad4(frames):
    """eval(): replicate-pad the bottom and the right up to a multiple of 4."""
    h, w = frames.shape[-2:]
    n, t, c = frames.shape[:3]
    x = F.pad(frames.reshape(n * t, c, h, w), (0, (-w) % 4, 0, (-h) % 4), mode="replicate")
    return x.reshape(n, t, c, x.shape[-2], x.shape[-1])


def loss(sd, frames, target, scale, max_flow=8.0, mc_weight=0.01, flow_weight=0.001):
    sr, mc, flow, _ = forward_terms(sd, frames, scale, max_flow)
    return ((sr - target) ** 2).mean() + mc_weight * mc + flow_weight * flow_huber(flow)


# -- the three-frame window over a stream (test_video) ------------------------------------------------------------------
def windows(T):
    """The frames output t is computed from."""
    return [(max(t - 1, 0), t, min(t + 1, T - 1)) for t in range(T)]


def output_batches(T, batch):
    """[(first, end)] output frames of each net call: reads of `batch` frames, output t needs frame t + 1 read (or the
    stream's end seen by a short read), so the output runs one frame behind and a short -- or empty -- read flushes."""
    out, read, done = [], 0, 0
    while True:
        k = min(batch, T - read)
        read += k
        end = T if k < batch else read - 1
        out.append((done, end))
        done = end
        if k < batch:
            return out


def packed_video(net, frames, W, H, sub, channels, batch, device):
    """The expected output frames [T, frame_bytes] of test_video: video_ref's front, `net` ([n,3,C,H,W] -> fp32 output) on
    the windows of every batch of output_batches, video_ref's tail with the chroma of the centre frames."""
    import numpy as np
    import video_ref as R
    T = len(frames)
    x = torch.from_numpy(R.unpack(frames, W, H, sub, channels))
    packed = []
    for a, b in output_batches(T, batch):
        if b == a:
            continue
        idx = torch.tensor(windows(T)[a:b])
        y = net(x[idx].to(device)).float().cpu().numpy()
        L = R.layout(y.shape[-1], y.shape[-2], sub)
        chroma = R.chroma_planes(frames[a:b], W, H, sub, L["cw"], L["ch"]) if (channels == 1 and sub != "mono") else None
        packed.append(R.pack(y, sub, chroma))
    return np.concatenate(packed), (y.shape[-1], y.shape[-2])
