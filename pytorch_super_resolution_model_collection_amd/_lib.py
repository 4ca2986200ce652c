"""ctypes binding of libsrk.so (the C ABI declared in include/srk.h).

There is deliberately NO fallback: if the library is missing or a call fails, a RuntimeError is
raised.  torch is used only for device memory, streams and autograd bookkeeping; every number on
the hot path is produced by a kernel in csrc/.

Nothing of the ABI is restated here: _header.py reads include/srk.h when this module is imported, and the constants
(SRK_X becomes X), the Structure fields and every function's restype / argtypes are its output.  One rule of that
reader shapes how the functions may be called: a pointer to an srk_ struct is POINTER(its Structure) -- an instance,
byref(x) or an array of them pass -- and EVERY other pointer parameter is c_void_p, host arrays included, because the
header does not say which side of the bus a `const int64_t*` lives on.  c_void_p takes ptr(t), None, a ctypes array, a
numpy data_as() result and byref(); what it no longer does is reject a pointer of the wrong element type.
"""
import ctypes
import os

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRK_LIB_PATH") or os.path.join(_HERE, "libsrk.so")  # env override: A/B kernel builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "srk.h")

MC_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "srk_mc.h")

_H = _header.read_file(HEADER_PATH)
_H_MC = _header.read_file(MC_HEADER_PATH)   # the motion-compensation entry points: a header of their own, the same reader
globals().update({name[len("SRK_"):]: value for name, value in _H.constants.items()})   # ACT_NONE, ALGO_MFMA, VERSION, ...
SSIM_DOMAINS = {"float": SSIM_FLOAT, "u8": SSIM_U8, "y8": SSIM_Y8}
ACT_BY_NAME = {None: ACT_NONE, "relu": ACT_RELU, "prelu": ACT_PRELU, "lrelu": ACT_LRELU, "tanh": ACT_TANH,
               "sigmoid": ACT_SIGMOID}


class _Sized:
    """a host out-struct the caller sizes through its leading struct_size"""

    def __init__(self):
        super().__init__()
        self.struct_size = ctypes.sizeof(type(self))


class ConvDesc(_H.classes["srk_conv_desc"]):
    """geometry of one Conv2d / ConvTranspose2d call"""


class Epilogue(_H.classes["srk_epilogue"]):
    """fused epilogue of a forward conv"""


class ConvResult(_Sized, _H.classes["srk_conv_result"]):
    """host out-struct of srk_conv2d_forward_ex"""


class BwdMask(_H.classes["srk_bwd_mask"]):
    """activation-gradient prologue of the backward kernels"""


class WgradPlan(_Sized, _H.classes["srk_wgrad_plan"]):
    """srk_conv2d_backward_weight_plan"""


class DenseDesc(_H.classes["srk_dense_desc"]):
    """a convolution over channel slices (csrc/dense.hip)"""


class DenseEpilogue(_Sized, _H.classes["srk_dense_epilogue"]):
    """the scaled output and the scaled skips of the srk_dense_conv_*_ex entry points"""

    def __init__(self, s=1.0, r1=1.0, r2=0.0, ldR2=0, a1=1.0):
        super().__init__()
        self.s, self.r1, self.r2, self.ldR2, self.a1 = float(s), float(r1), float(r2), int(ldR2), float(a1)


class DensePlan(_Sized, _H.classes["srk_dense_plan"]):
    """srk_dense_conv_plan"""


class SpectralLayer(_H.classes["srk_spectral_layer"]):
    """srk_spectral_norm_forward"""


class PhaseAxis(_Sized, _H.classes["srk_phase_axis"]):
    """srk_trans_phase_axis"""


class Phase(_Sized, _H.classes["srk_phase"]):
    """srk_trans_phases"""


_PROTOTYPES = _H.functions   # {name: (restype, [argtypes])}
_MC_PROTOTYPES = _H_MC.functions   # the same for include/srk_mc.h

_lib = None


def header_symbols():
    """Every function name declared in include/srk.h."""
    return sorted(_PROTOTYPES)


def mc_header_symbols():
    """Every function name declared in include/srk_mc.h."""
    return sorted(_MC_PROTOTYPES)


def load():
    """Load libsrk.so (building it is __graft_entry__.build()'s job). Raises if it is missing or not the header's version."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libsrk.so not found at %s — run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950). "
            "There is no CPU/eager fallback for the hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(_PROTOTYPES.items()) + list(_MC_PROTOTYPES.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.srk_version() != VERSION:
        raise RuntimeError("%s is version %d but %s declares SRK_VERSION %d: a stale library beside a newer header (or the "
                           "reverse) -- rebuild with `python __graft_entry__.py build`"
                           % (LIB_PATH, lib.srk_version(), HEADER_PATH, VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        lib = load()
        raise RuntimeError("%s failed: %s (%s)" % (what, lib.srk_status_string(rc).decode(),
                                                   lib.srk_last_error_string().decode()))


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "the MI355X hot path only runs on GPU tensors (got a %s tensor); there is no CPU fallback — "
                "use oracle/ for a CPU reference" % t.device)
        if t is not None and t.device.index is not None and t.device.index != torch.cuda.current_device():
            # kernels are enqueued on the CURRENT device's stream (one process per GPU): a tensor of another device
            # would be dereferenced by the wrong GPU
            raise RuntimeError("tensor on %s but the current device is cuda:%d — call torch.cuda.set_device(%d) (one "
                               "process per GPU) or wrap the call in torch.cuda.device(...)"
                               % (t.device, torch.cuda.current_device(), t.device.index))
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("the hot path is fp32 (got %s)" % t.dtype)
