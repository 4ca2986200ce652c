"""The x8 geometric self-ensemble as its definition reads, with stock torch ops, for the tests: the eight
torch.rot90 / torch.flip calls around any callable `f` (an oracle.ref_modules net on the CPU, or the identity).

    k = 4 m + r      T_k(x) = rot90(flip(x, -1) if m else x, r, (-2, -1))      T_k^-1(y) = flip_m(rot90(y, -r, (-2, -1)))
    E(x) = (((((((y_0 + y_1) + y_2) + y_3) + y_4) + y_5) + y_6) + y_7) * 0.125,      y_k = T_k^-1(f(T_k(x)))
"""
import torch


def transform(x, k):
    m, r = divmod(k, 4)
    return torch.rot90(torch.flip(x, (-1,)) if m else x, r, (-2, -1))


def inverse(y, k):
    m, r = divmod(k, 4)
    y = torch.rot90(y, -r, (-2, -1))
    return torch.flip(y, (-1,)) if m else y


def _last(out):
    return out[-1] if isinstance(out, (tuple, list)) else out


def terms(f, x):
    """[y_0 .. y_7] for the net input x [N,C,H,W]."""
    with torch.no_grad():
        return [inverse(_last(f(transform(x, k).contiguous())), k) for k in range(8)]


def mean_in_order(ys):
    """the seven adds in order, then * 0.125, in the dtype of the terms"""
    acc = ys[0]
    for y in ys[1:]:
        acc = acc + y
    return acc * 0.125


def ensemble(f, x):
    return mean_in_order(terms(f, x))


def groups(ys_before_inverse):
    """[f(T_0 x) .. f(T_7 x)] for N pictures -> (even [4N,...], odd [4N,...]) in the order ops.dihedral_merge takes:
    image 4 n + j of even is k = (0, 2, 4, 6)[j] of picture n, of odd k = (1, 3, 5, 7)[j]."""
    n = ys_before_inverse[0].shape[0]
    even = torch.stack([ys_before_inverse[k][i] for i in range(n) for k in (0, 2, 4, 6)])
    odd = torch.stack([ys_before_inverse[k][i] for i in range(n) for k in (1, 3, 5, 7)])
    return even, odd
