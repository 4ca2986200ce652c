"""TEST INFRASTRUCTURE shared by the convolution tests that go through the C ABI (tests/test_strided_gpu.py,
tests/test_stride1_epilogue_gpu.py): tensors cut from one flat allocation at a chosen byte offset past a 16-byte boundary,
outputs between sentinel guards, and the share of assert_close_elementwise's bar that a result uses."""
import numpy as np
import torch

GUARD = 64
SENT = -12345.5


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _edges_x4(t):
    """NCHW tensor with its outermost two rows and columns multiplied by 4"""
    H, W = t.shape[2], t.shape[3]
    m = torch.ones(H, W)
    m[:2], m[-2:], m[:, :2], m[:, -2:] = 4.0, 4.0, 4.0, 4.0
    return t * m


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _place(t, gpu, off=0):
    """a flat device copy of t, `off` bytes past a 16-byte boundary inside one allocation"""
    assert off % 4 == 0 and 0 <= off < 16
    flat = t.reshape(-1)
    big = torch.empty(flat.numel() + 4, dtype=torch.float32, device=gpu)
    assert big.data_ptr() % 16 == 0
    v = big[off // 4: off // 4 + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == off and v.numel() == flat.numel()
    return v


class Guarded(object):
    """n floats `off` bytes past a 16-byte boundary inside one allocation, at least GUARD sentinel floats either side;
    NaN-filled, or filled with `init`"""

    def __init__(self, n, gpu, off=0, init=None):
        self.n, self.lo = n, GUARD + off // 4
        self.big = torch.full((GUARD + n + GUARD + 4,), SENT, dtype=torch.float32, device=gpu)
        self.t = self.big[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == off
        self.t.fill_(float("nan") if init is None else init)

    def check(self, what):
        big = self.big.cpu().numpy()
        lo, hi = self.lo, self.lo + self.n
        assert (big[:lo] == np.float32(SENT)).all() and (big[hi:] == np.float32(SENT)).all(), "%s: a guard was written" % what
        assert not np.isnan(big[lo:hi]).any(), "%s: %d elements never written" % (what, int(np.isnan(big[lo:hi]).sum()))
        return big[lo:hi].copy()

    def check_untouched(self, what):
        """a refused call: the guards intact and every element still NaN"""
        big = self.big.cpu().numpy()
        lo, hi = self.lo, self.lo + self.n
        assert (big[:lo] == np.float32(SENT)).all() and (big[hi:] == np.float32(SENT)).all(), "%s: a guard was written" % what
        assert np.isnan(big[lo:hi]).all(), "%s: %d elements were written" % (what, int((~np.isnan(big[lo:hi])).sum()))


def _ratio(got, ref, rtol):
    """worst |got - ref| / (atol + rtol |ref|), atol = rtol * rms(ref): how much of assert_close_elementwise's bar is used"""
    ref = np.asarray(ref, np.float64)
    atol = rtol * float(np.sqrt(np.mean(ref * ref)))
    return float((np.abs(np.asarray(got, np.float64) - ref) / (atol + rtol * np.abs(ref))).max())
