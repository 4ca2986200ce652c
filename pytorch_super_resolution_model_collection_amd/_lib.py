"""ctypes binding of libsrk.so (the C ABI declared in include/srk.h).

There is deliberately NO fallback: if the library is missing or a call fails, a RuntimeError is
raised.  torch is used only for device memory, streams and autograd bookkeeping; every number on
the hot path is produced by a kernel in csrc/.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRK_LIB_PATH") or os.path.join(_HERE, "libsrk.so")  # env override: A/B kernel builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "srk.h")

# enums mirrored from include/srk.h
ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = range(6)
ALGO_AUTO, ALGO_GENERIC, ALGO_MFMA, ALGO_DIRECT, ALGO_MFMA_BF16X3, ALGO_MFMA_BF16X6, ALGO_MFMA_F16X3 = range(7)
AMAX_FLOATS = 256   # SRK_AMAX_FLOATS: 16 slots, one per 64-byte line
LOSS_MSE, LOSS_L1, LOSS_CHARBONNIER, LOSS_BCE = range(4)
FFT_LOSS_MAX_DIM = 256   # SRK_FFT_LOSS_MAX_DIM
VGG_TAP_POOL, VGG_TAP_RELU, VGG_TAP_LAST = range(3)   # srk_vgg_tap_mode
SSIM_DOMAINS = {"float": 0, "u8": 1, "y8": 2}   # SRK_SSIM_FLOAT / _U8 / _Y8
NIQE_TABLE, NIQE_FEATURES = 9801, 36   # SRK_NIQE_TABLE / SRK_NIQE_FEATURES
ACT_BY_NAME = {None: ACT_NONE, "relu": ACT_RELU, "prelu": ACT_PRELU, "lrelu": ACT_LRELU, "tanh": ACT_TANH,
               "sigmoid": ACT_SIGMOID}

c_f = ctypes.c_void_p  # device float*
c_vp = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size = ctypes.c_size_t


class ConvDesc(ctypes.Structure):
    """struct srk_conv_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("N", "H", "W", "Cin", "OH", "OW", "Cout", "KH", "KW", "stride", "pad", "transposed", "out_pad",
                 "algo", "x_nchw", "dy_ps_r")]


class Epilogue(ctypes.Structure):
    """struct srk_epilogue"""
    _fields_ = [("bias", c_vp), ("prelu_weight", c_vp), ("residual", c_vp), ("slope", c_float),
                ("act", ctypes.c_int32), ("prelu_n", ctypes.c_int32), ("ps_r", ctypes.c_int32),
                ("x_amax", c_vp), ("y_amax", c_vp), ("bn_partial", c_vp)]


class ConvResult(ctypes.Structure):
    """struct srk_conv_result (host out-struct of srk_conv2d_forward_ex; struct_size is the caller's sizeof)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("wrote_amax", ctypes.c_int32), ("bn_partial_rows", ctypes.c_int32)]

    def __init__(self):
        super().__init__(ctypes.sizeof(ConvResult), 0, 0)


class BwdMask(ctypes.Structure):
    """struct srk_bwd_mask"""
    _fields_ = [("y", c_vp), ("slope", c_float)]


class _Sized(ctypes.Structure):
    """a host out-struct the caller sizes through its leading struct_size"""

    def __init__(self):
        super().__init__()
        self.struct_size = ctypes.sizeof(type(self))


class WgradPlan(_Sized):
    """struct srk_wgrad_plan (srk_conv2d_backward_weight_plan)"""
    _fields_ = ([("struct_size", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in
                ("ok", "kernel", "cfg", "CIB", "COB", "spec", "k33", "prefetch", "ring", "vec_x", "vec_y", "scalar",
                 "grouped", "n", "G", "grid_x", "grid_y", "grid_z", "block", "lds_bytes", "TH", "TW", "TWo", "HH", "HWp",
                 "CS", "DS", "nks", "tiles_y", "tiles_x", "ntiles", "gy", "gz", "lds_set", "ring_bytes", "XP", "XPL", "YPL")]
                + [("slab_bytes", ctypes.c_uint64), ("ws_bytes", ctypes.c_uint64), ("name", ctypes.c_char * 64)])


class DenseDesc(ctypes.Structure):
    """struct srk_dense_desc: a convolution over channel slices (csrc/dense.hip)"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("N", "H", "W", "K", "CA", "CB", "Cout", "ldA", "ldB", "ldY", "ldR", "ldDy",
                                               "ldDA", "ldDB", "ldAdd", "act")]
                + [("slope", c_float), ("terms", ctypes.c_int32)])


class DenseEpilogue(_Sized):
    """struct srk_dense_epilogue: the scaled output and the scaled skips of the srk_dense_conv_*_ex entry points"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("s", c_float), ("r1", c_float), ("r2", c_float), ("ldR2", ctypes.c_int32),
                ("a1", c_float)]

    def __init__(self, s=1.0, r1=1.0, r2=0.0, ldR2=0, a1=1.0):
        super().__init__()
        self.s, self.r1, self.r2, self.ldR2, self.a1 = float(s), float(r1), float(r2), int(ldR2), float(a1)


class DensePlan(_Sized):
    """struct srk_dense_plan (srk_dense_conv_plan)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("pix_tiles", ctypes.c_int32), ("splits", ctypes.c_int32),
                ("split_pixels", ctypes.c_int64), ("ws_bytes", ctypes.c_uint64), ("partial_floats", ctypes.c_uint64)]


SPECTRAL_MAX_LAYERS = 16   # SRK_SPECTRAL_MAX_LAYERS


class SpectralLayer(ctypes.Structure):
    """struct srk_spectral_layer (srk_spectral_norm_forward)"""
    _fields_ = [("W", c_vp), ("u", c_vp), ("v", c_vp), ("w_sn", c_vp), ("saved", c_vp), ("R", ctypes.c_int32),
                ("K", ctypes.c_int32)]


class PhaseAxis(_Sized):
    """struct srk_phase_axis (srk_trans_phase_axis)"""
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in ("o0", "P", "Kv", "i0", "w0", "wd")]


class Phase(_Sized):
    """struct srk_phase (srk_trans_phases)"""
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in
                ("oy0", "ox0", "PH", "PW", "KHv", "KWv", "iy0", "ix0", "wh0", "wdh", "ww0", "wdw")]


_PROTOTYPES = {
    "srk_version": (c_int, []),
    "srk_status_string": (ctypes.c_char_p, [c_int]),
    "srk_last_error_string": (ctypes.c_char_p, []),
    "srk_last_kernel_name": (ctypes.c_char_p, []),
    "srk_last_conv_wrote_amax": (c_int, []),
    "srk_last_conv_bn_partial_rows": (c_int, []),
    "srk_ring_timeouts": (c_int, [c_int]),
    "srk_conv_out_dim": (c_int, [c_int] * 6),
    "srk_conv2d_backward_weight_plan": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_int, c_int, c_int,
                                                ctypes.POINTER(WgradPlan)]),
    "srk_trans_phase_axis": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(PhaseAxis), c_int]),
    "srk_trans_phases": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(Phase), c_int]),
    "srk_nchw_to_nhwc": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "srk_nhwc_to_nchw": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "srk_pack_weight_fwd": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_pack_weight_bwd": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_pack_bias_ps": (c_int, [c_f, c_f, c_int, c_int, c_vp]),
    "srk_wgrad_reduce_defer": (c_int, [c_int]),
    "srk_wgrad_reduce_flush": (c_int, [c_vp]),
    "srk_pack_weights_batched": (c_int, [c_f, c_vp, c_vp, c_int, c_int, c_vp, c_int, c_vp]),
    "srk_packed_weight_bytes": (c_size, [c_int, c_int, c_int, c_int, c_int]),
    "srk_conv2d_forward": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, c_f, ctypes.POINTER(Epilogue), c_vp]),
    "srk_conv2d_forward_ex": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, c_f, ctypes.POINTER(Epilogue),
                                      ctypes.POINTER(ConvResult), c_vp]),
    "srk_conv2d_backward_data": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, c_f, ctypes.POINTER(BwdMask), c_f,
                                         c_vp]),
    "srk_conv2d_backward_data_relu_supported": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, ctypes.POINTER(BwdMask)]),
    "srk_conv2d_backward_data_relu": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, c_f, ctypes.POINTER(BwdMask), c_f,
                                              c_vp]),
    "srk_conv2d_backward_weight_workspace_bytes": (c_size, [ctypes.POINTER(ConvDesc)]),
    "srk_conv2d_backward_weight": (c_int, [ctypes.POINTER(ConvDesc), c_f, c_f, ctypes.POINTER(BwdMask), c_f, c_f,
                                           c_float, c_vp, c_size, c_vp]),
    "srk_conv2d_backward_weight_grouped_workspace_bytes": (c_size, [ctypes.POINTER(ConvDesc), c_int]),
    "srk_conv2d_backward_weight_grouped": (c_int, [ctypes.POINTER(ConvDesc), c_int, ctypes.POINTER(c_vp),
                                                   ctypes.POINTER(c_vp), ctypes.POINTER(BwdMask), ctypes.POINTER(c_vp),
                                                   ctypes.POINTER(c_vp), c_float, c_vp, c_size, c_vp]),
    "srk_resblock2_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "srk_espcn_pair_prepared_bytes": (c_size, []),
    "srk_espcn_pair_prepare": (c_int, [c_f, c_f, c_vp, c_vp]),
    "srk_espcn_pair_forward": (c_int, [c_int, c_int, c_int, c_f, c_vp, c_f, c_f, c_f, c_f, c_f, c_int, c_f, c_int, c_vp]),
    "srk_espcn_pair_scans": (c_int, [c_int]),
    "srk_resblock2_forward": (c_int, [c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_int, c_f, c_f,
                                      c_vp]),
    "srk_absmax": (c_int, [c_f, c_size, c_f, c_vp]),
    "srk_conv2d_f16x3_supported": (c_int, [ctypes.POINTER(ConvDesc), ctypes.POINTER(Epilogue), c_f]),
    "srk_resblock2_backward_data": (c_int, [c_int, c_int, c_int, c_int, c_f, c_f, c_f, c_f, c_f, c_f, c_int, c_vp]),
    "srk_pixel_shuffle_forward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_pixel_shuffle_backward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_act_forward": (c_int, [c_f, c_f, c_size, c_int, c_int, c_float, c_f, c_int, c_vp]),
    "srk_act_backward": (c_int, [c_f, c_f, c_f, c_size, c_int, c_int, c_float, c_f, c_int, c_f, c_vp]),
    "srk_axpby": (c_int, [c_f, c_f, c_f, c_size, c_float, c_float, c_vp]),
    "srk_loss_workspace_bytes": (c_size, []),
    "srk_loss_forward_backward": (c_int, [c_int, c_f, c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int,
                                          c_int, c_float, c_float, c_f, c_f, c_vp, c_vp]),
    "srk_drcn_head_forward": (c_int, [c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_f, c_vp]),
    "srk_drcn_workspace_bytes": (c_size, [c_int]),
    "srk_drcn_head_loss": (c_int, [c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_f, c_f, c_float, c_f, c_f,
                                   c_f, c_f, c_f, c_float, c_vp, c_size, c_vp]),
    "srk_drcn_head_backward": (c_int, [c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_f, c_f, c_float, c_vp, c_size,
                                       c_vp]),
    "srk_sumsq_workspace_bytes": (c_size, []),
    "srk_sumsq": (c_int, [c_f, c_size, c_float, c_f, c_vp, c_vp]),
    "srk_sgd_step": (c_int, [c_f, c_f, c_f, c_size, c_float, c_float, c_float, c_int, c_int, c_f, c_f, c_vp]),
    "srk_adam_step": (c_int, [c_f, c_f, c_f, c_f, c_size, c_float, c_float, c_float, c_float, c_float, c_vp, c_f,
                              c_f, c_vp]),
    "srk_sgd_step_ema": (c_int, [c_f, c_f, c_f, c_size, c_float, c_float, c_float, c_int, c_int, c_f, c_f, c_f, c_float,
                                 c_vp]),
    "srk_adam_step_ema": (c_int, [c_f, c_f, c_f, c_f, c_size, c_float, c_float, c_float, c_float, c_float, c_vp, c_f,
                                  c_f, c_f, c_float, c_vp]),
    "srk_grad_norm_workspace_bytes": (c_size, []),
    "srk_grad_norm_clip": (c_int, [c_f, c_size, c_float, c_f, c_f, c_vp, c_vp]),
    "srk_bn_stats": (c_int, [c_f, c_vp, c_size, c_int, c_vp, c_vp]),
    "srk_bn_workspace_bytes": (c_size, [c_int]),
    "srk_bn_finalize": (c_int, [c_vp, ctypes.c_double, c_f, c_f, c_f, c_f, c_float, c_float, c_int, c_vp, c_vp]),
    "srk_bn_stats_finalize": (c_int, [c_f, c_vp, c_size, c_int, c_f, c_f, c_f, c_f, c_float, c_float, c_vp, c_vp, c_vp]),
    "srk_bn_finalize_partials": (c_int, [c_vp, c_int, c_vp, c_size, c_int, c_f, c_f, c_f, c_f, c_float, c_float, c_vp, c_vp]),
    "srk_bn_backward_stats_grads": (c_int, [c_f, c_f, c_f, c_f, c_vp, c_size, c_int, c_f, c_f, c_vp, c_vp]),
    "srk_bn_apply": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_size, c_int, c_int, c_float, c_f, c_vp]),
    "srk_bn_apply_act": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_size, c_int, c_int, c_float, c_f, c_int, c_f, c_f, c_vp]),
    "srk_bn_backward_stats_grads_act": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_vp, c_size, c_int, c_f, c_f, c_int,
                                                 c_float, c_f, c_int, c_f, c_vp, c_vp]),
    "srk_bn_backward_apply_act": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_vp, ctypes.c_double, c_f, c_size, c_int, c_int,
                                           c_float, c_f, c_int, c_vp]),
    "srk_bn_fused_supported": (c_int, [c_int]),
    "srk_bn_stats_partials": (c_int, [c_f, c_size, c_int, c_vp, ctypes.POINTER(c_int), c_vp]),
    "srk_bn_finalize_apply_act": (c_int, [c_vp, c_int, c_vp, c_size, c_int, c_f, c_f, c_f, c_f, c_float, c_float, c_vp,
                                          c_f, c_f, c_f, c_f, c_int, c_float, c_f, c_int, c_f, c_f, c_vp]),
    "srk_bn_backward_partials_act": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_size, c_int, c_int, c_float, c_f, c_int, c_vp,
                                             ctypes.POINTER(c_int), c_vp]),
    "srk_bn_backward_finalize_apply_act": (c_int, [c_vp, c_int, c_vp, ctypes.c_double, c_f, c_f, c_f, c_f, c_f, c_f, c_f,
                                                   c_size, c_int, c_f, c_f, c_int, c_float, c_f, c_int, c_f, c_vp]),
    "srk_bn_eval_params": (c_int, [c_f, c_f, c_float, c_f, c_f, c_int, c_vp]),
    "srk_rownorm_forward": (c_int, [c_f, c_f, c_f, c_f, c_int, c_int, c_float, c_vp]),
    "srk_rownorm_backward": (c_int, [c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_vp]),
    "srk_bn_backward_stats": (c_int, [c_f, c_f, c_f, c_f, c_vp, c_size, c_int, c_vp, c_vp]),
    "srk_bn_backward_apply": (c_int, [c_f, c_f, c_f, c_f, c_f, c_vp, ctypes.c_double, c_f, c_size, c_int, c_vp]),
    "srk_bn_param_grads": (c_int, [c_vp, c_f, c_f, c_int, c_vp]),
    "srk_scale_dev": (c_int, [c_f, c_f, c_f, c_size, c_vp]),
    "srk_linear_forward": (c_int, [c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_float, c_vp]),
    "srk_linear_backward": (c_int, [c_f, c_f, c_f, c_f, c_f, c_f, c_int, c_int, c_int, c_float, c_vp]),
    "srk_img_resize_u8_workspace_bytes": (c_size, [c_int] * 6),
    "srk_img_resize_u8": (c_int, [c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_int, c_vp, c_size, c_vp]),
    "srk_patch_augment_u8": (c_int, [c_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_int, c_int, c_int,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_patch_from_image_u8_workspace_bytes": (c_size, [c_int, c_int, c_int, c_int, c_int]),
    "srk_patch_from_image_u8": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_vp, c_vp, c_size, c_vp]),
    "srk_rgb_to_ycc_u8": (c_int, [c_vp, ctypes.c_int64, c_int, c_int, c_f, c_vp, c_vp, c_vp]),
    "srk_ycc_to_rgb_u8": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp]),
    "srk_float_to_u8_image": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_vp, c_int, c_int, c_int, c_vp]),
    "srk_tile_gather": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_f, c_vp]),
    "srk_tile_stitch_f32": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_f, c_int, c_int, c_vp]),
    "srk_tile_stitch_u8": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_vp]),
    "srk_dihedral_variants": (c_int, [c_f, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int, c_int, c_f, c_vp]),
    "srk_dihedral_merge_f32": (c_int, [c_f, ctypes.POINTER(ctypes.c_int64), c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_int, c_f, c_vp]),
    "srk_dihedral_merge_u8": (c_int, [c_f, ctypes.POINTER(ctypes.c_int64), c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp]),
    "srk_rgb_to_ycc_host": (c_int, [c_vp, c_size, c_vp]),
    "srk_ycc_to_rgb_host": (c_int, [c_vp, c_size, c_vp]),
    "srk_psnr_workspace_bytes": (c_size, []),
    "srk_psnr": (c_int, [c_f, ctypes.POINTER(ctypes.c_int64), c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int,
                         c_int, c_f, c_f, c_vp, c_vp]),
    "srk_ssim_workspace_bytes": (c_size, []),
    "srk_ssim": (c_int, [c_f, ctypes.POINTER(ctypes.c_int64), c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int,
                         c_int, c_int, c_int, c_f, c_f, c_f, c_vp, c_vp]),
    "srk_ssim_host": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int64), c_vp, ctypes.POINTER(ctypes.c_int64), c_int, c_int,
                              c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                              ctypes.POINTER(ctypes.c_double)]),
    "srk_ssim_loss_workspace_bytes": (c_size, []),
    "srk_ssim_loss_forward_backward": (c_int, [c_f, c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_int,
                                               c_float, c_f, c_f, c_vp, c_vp]),
    "srk_ssim_loss_host": (c_int, [c_vp, c_vp, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_int,
                                   ctypes.c_double, ctypes.POINTER(ctypes.c_double), c_vp]),
    "srk_dft_table_host": (c_int, [c_int, ctypes.POINTER(ctypes.c_double)]),
    "srk_fft_loss_workspace_bytes": (c_size, [c_int, c_int, c_int, c_int]),
    "srk_fft_loss_forward_backward": (c_int, [c_f, c_f, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_int, c_vp,
                                              ctypes.c_double, c_float, c_f, c_f, c_vp, c_vp]),
    "srk_fft_loss_host": (c_int, [c_vp, c_vp, ctypes.POINTER(ctypes.c_int64), c_int, c_int, c_int, c_int, ctypes.c_double,
                                  ctypes.c_double, ctypes.POINTER(ctypes.c_double), c_vp]),
    "srk_channel_affine": (c_int, [c_f, c_f, c_size, c_int, c_size, ctypes.POINTER(c_float), ctypes.POINTER(c_float),
                                   c_int, c_vp]),
    "srk_upsample_nearest_forward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_upsample_nearest_backward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_maxpool2x2_forward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "srk_maxpool2x2_backward": (c_int, [c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_img_interp_workspace_bytes": (ctypes.c_size_t, [c_int] * 7),
    "srk_img_interp": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, ctypes.c_size_t, c_vp]),
    "srk_blur_u8": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_noise_u8": (c_int, [c_vp, c_f, c_vp, ctypes.c_uint64, c_int, ctypes.c_int64, c_vp]),
    "srk_blur_weights_host": (c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int,
                                      ctypes.POINTER(ctypes.c_double)]),
    "srk_noise_normals_host": (c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]),
    "srk_philox4x32_10_host": (c_int, [ctypes.POINTER(ctypes.c_uint32)] * 3),
    "srk_jpeg_u8": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "srk_noise_u8_bytes": (c_int, [c_vp, c_vp, c_vp, ctypes.c_uint64, c_int, ctypes.c_int64, c_vp]),
    "srk_jpeg_quant_table_host": (c_int, [c_int, c_int, ctypes.POINTER(c_int)]),
    "srk_jpeg_u8_host": (c_int, [c_vp, c_vp, ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int]),
    "srk_channel_attention_splits": (c_int, [c_int] * 4),
    "srk_channel_attention_workspace": (c_size, [c_int] * 4),
    "srk_channel_attention_forward": (c_int, [c_f] * 6 + [c_int] * 5 + [c_f] * 4 + [c_vp, c_size, c_vp]),
    "srk_channel_attention_backward": (c_int, [c_f] * 7 + [c_int] * 5 + [c_f] * 5 + [c_float, c_vp, c_size, c_vp]),
    "srk_channel_attention_host": (c_int, [c_vp] * 7 + [c_int] * 5 + [c_vp] * 6),
    "srk_lpips_layer_workspace": (c_size, [c_int] * 4),
    "srk_lpips_layer_blocks": (c_int, [c_int] * 5),
    "srk_lpips_layer_forward": (c_int, [c_f] * 3 + [c_int] * 6 + [c_vp, c_vp, c_size, c_vp]),
    "srk_lpips_finish": (c_int, [c_vp, c_int, c_int, ctypes.c_double, c_f, c_f, c_vp, c_vp]),
    "srk_lpips_layer_backward": (c_int, [c_f] * 3 + [c_vp] + [c_int] * 4 + [c_f, c_vp]),
    "srk_lpips_layer_host": (c_int, [c_vp] * 4 + [c_int] * 4 + [c_vp] * 2),
    "srk_dense_conv_supported": (c_int, [ctypes.POINTER(DenseDesc)]),
    "srk_dense_conv_plan": (c_int, [ctypes.POINTER(DenseDesc), ctypes.POINTER(DensePlan)]),
    "srk_dense_conv_workspace_bytes": (c_size, [ctypes.POINTER(DenseDesc)]),
    "srk_dense_conv_forward": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 6 + [c_vp]),
    "srk_dense_conv_backward_data": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 4 + [c_float, c_f, c_float, c_f, c_vp]),
    "srk_dense_conv_backward_weight": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 6 + [c_float, c_vp, c_size, c_vp]),
    "srk_dense_conv_host": (c_int, [ctypes.POINTER(DenseDesc), c_int] + [c_vp] * 9 + [c_float, c_vp, c_float, c_vp, c_vp,
                                                                                     c_float]),
    "srk_dense_conv_forward_ex": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 6 + [ctypes.POINTER(DenseEpilogue), c_f, c_vp]),
    "srk_dense_conv_backward_data_ex": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 4 + [c_float, c_f, c_float, c_f,
                                                                                         ctypes.POINTER(DenseEpilogue), c_vp]),
    "srk_dense_conv_backward_weight_ex": (c_int, [ctypes.POINTER(DenseDesc)] + [c_f] * 6 + [c_float, ctypes.POINTER(DenseEpilogue),
                                                                                           c_vp, c_size, c_vp]),
    "srk_dense_conv_host_ex": (c_int, [ctypes.POINTER(DenseDesc), c_int] + [c_vp] * 6 + [ctypes.POINTER(DenseEpilogue)]
                               + [c_vp] * 4 + [c_float, c_vp, c_float, c_vp, c_vp, c_float]),
    "srk_ragan_loss_forward_backward": (c_int, [c_f, c_f, c_int, c_int, c_float, c_f, c_f, c_f, c_vp, c_vp]),
    "srk_ragan_loss_host": (c_int, [c_vp, c_vp, c_int, c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double), c_vp, c_vp]),
    "srk_window_attention_workspace": (c_size, [c_int] * 6),
    "srk_window_attention_forward": (c_int, [c_f, c_f] + [c_int] * 7 + [c_f, c_f, c_vp]),
    "srk_window_attention_backward": (c_int, [c_f] * 5 + [c_int] * 7 + [c_f, c_f, c_float, c_vp, c_size, c_vp]),
    "srk_window_attention_host": (c_int, [c_vp] * 3 + [c_int] * 7 + [c_vp] * 3),
    "srk_window_attention_region": (c_int, [c_int] * 6),
    "srk_window_attention_rel_index": (c_int, [c_int] * 3),
    "srk_window_attention_token_pixel": (ctypes.c_int64, [c_int] * 7),
    "srk_layer_norm_workspace": (c_size, [ctypes.c_int64, c_int]),
    "srk_layer_norm_forward": (c_int, [c_f] * 6 + [ctypes.c_int64, c_int, c_float, c_vp]),
    "srk_layer_norm_backward": (c_int, [c_f] * 8 + [c_float, ctypes.c_int64, c_int, c_vp, c_size, c_vp]),
    "srk_gelu_forward": (c_int, [c_f, c_f, c_size, c_vp]),
    "srk_gelu_backward": (c_int, [c_f, c_f, c_f, c_size, c_vp]),
    "srk_spectral_norm_workspace": (c_size, [ctypes.POINTER(SpectralLayer), c_int]),
    "srk_spectral_norm_forward": (c_int, [ctypes.POINTER(SpectralLayer), c_int, c_int, ctypes.c_double, c_vp, c_size, c_vp]),
    "srk_spectral_norm_backward_workspace": (c_size, [c_int, c_int]),
    "srk_spectral_norm_backward": (c_int, [c_f, c_f, c_f, c_int, c_int, c_f, c_float, c_vp, c_size, c_vp]),
    "srk_spectral_norm_host": (c_int, [c_vp, c_int, c_int, c_int, ctypes.c_double, c_vp, c_vp, c_vp,
                                       ctypes.POINTER(ctypes.c_double), c_vp, c_vp]),
    "srk_upsample_bilinear2x_forward": (c_int, [c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "srk_upsample_bilinear2x_backward": (c_int, [c_f, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "srk_upsample_bilinear2x_host": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "srk_gan_logit_loss_workspace_bytes": (c_size, []),
    "srk_gan_logit_loss_forward_backward": (c_int, [c_f, c_size, c_int, c_float, c_f, c_f, c_vp, c_vp]),
    "srk_gan_logit_loss_host": (c_int, [c_vp, c_size, c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double), c_vp]),
    "srk_blur_table_host": (c_int, [c_int, c_int] + [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_double)]),
    "srk_poisson_cdf_host": (c_int, [ctypes.c_double, c_int, c_vp]),
    "srk_noise2_u8": (c_int, [c_vp] * 6 + [ctypes.c_uint64] + [c_int] * 6 + [c_vp]),
    "srk_noise2_u8_host": (c_int, [c_vp] * 6 + [ctypes.c_uint64] + [c_int] * 6),
    "srk_usm_table_host": (c_int, [c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "srk_usm_u8_workspace_bytes": (c_size, [c_int] * 4),
    "srk_usm_u8": (c_int, [c_vp] * 3 + [c_int, ctypes.c_double, ctypes.c_double] + [c_int] * 4 + [c_vp, c_size, c_vp]),
    "srk_usm_u8_host": (c_int, [c_vp] * 3 + [c_int, ctypes.c_double, ctypes.c_double] + [c_int] * 4),
    "srk_vgg_tap_workspace_bytes": (c_size, [c_int]),
    "srk_vgg_tap_plan": (c_int, [c_int] * 6 + [ctypes.POINTER(ctypes.c_longlong)]),
    "srk_vgg_tap_forward": (c_int, [c_f, c_f] + [c_int] * 5 + [ctypes.c_double, c_int, c_int, c_vp, c_f, c_f, c_vp]),
    "srk_vgg_tap_finish": (c_int, [c_vp, c_int, c_f, c_vp]),
    "srk_vgg_tap_backward": (c_int, [c_f] * 3 + [c_int] * 5 + [ctypes.c_double, c_f, c_f, c_vp]),
    "srk_vgg_tap_forward_host": (c_int, [c_vp, c_vp] + [c_int] * 5 + [ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                         c_vp, c_vp]),
    "srk_vgg_tap_backward_host": (c_int, [c_vp] * 3 + [c_int] * 5 + [ctypes.c_double, c_vp]),
    "srk_niqe_tables_host": (c_int, [ctypes.POINTER(ctypes.c_double)]),
    "srk_niqe_workspace_bytes": (c_size, [c_int] * 3),
    "srk_niqe_features": (c_int, [c_vp, c_int, ctypes.POINTER(ctypes.c_int64)] + [c_int] * 5 + [c_vp] * 5),
    "srk_niqe_features_host": (c_int, [c_vp, c_int, ctypes.POINTER(ctypes.c_int64)] + [c_int] * 5 + [c_vp] * 3),
    "srk_yuv_unpack": (c_int, [c_vp, ctypes.c_int64] + [c_int] * 5 + [c_vp] * 3),
    "srk_yuv_pack": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int64)] + [c_int] * 5 + [c_vp, c_vp, ctypes.c_int64, c_vp]),
    "srk_yuv_unpack_host": (c_int, [c_vp, ctypes.c_int64] + [c_int] * 5 + [c_vp] * 2),
    "srk_yuv_pack_host": (c_int, [c_vp, ctypes.POINTER(ctypes.c_int64)] + [c_int] * 5 + [c_vp, c_vp, ctypes.c_int64]),
}

_lib = None


def header_symbols():
    """Every function name declared in include/srk.h (used by the CPU-side export test)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srk_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load libsrk.so (building it is __graft_entry__.build()'s job). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libsrk.so not found at %s — run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950). "
            "There is no CPU/eager fallback for the hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


ERR_UNSUPPORTED = -2   # SRK_ERR_UNSUPPORTED (include/srk.h)


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
