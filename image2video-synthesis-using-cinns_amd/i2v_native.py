"""ctypes binding of ``libi2v_hip.so`` (C ABI declared in ``include/i2v_hip.h``).

PyTorch-ROCm tensors are used only as containers: every call passes raw device pointers
(``tensor.data_ptr()``) and the current HIP stream.  There is NO CPU fallback: if the shared
library is missing, or a tensor does not live on a GPU, the call raises.
"""
import ctypes
import weakref
import functools
import os
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libi2v_hip.so")
if os.environ.get("I2V_LIB_PATH"):   # measurement: another build of the same library (tools/build_measurement_libs.sh), relative to the repo
    LIB_PATH = os.path.join(os.path.dirname(_PKG), os.environ["I2V_LIB_PATH"])
CSRC = os.path.join(_PKG, "csrc")

I2V_F32, I2V_I64, I2V_U8 = 0, 1, 2


class I2VError(RuntimeError):
    pass


class _Tensor(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", c_void_p), ("numel", c_int64), ("dtype", c_int32)]


class FlowCfg(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("in_channels", "embedding_dim", "hidden_dim", "hidden_depth", "n_flows",
                                      "control", "activation", "skip_actnorm", "skip_shuffle", "use_graph", "linear_f16")]


class FlowTrainLayout(ctypes.Structure):
    _fields_ = [(n, c_int64) for n in ("KP", "step_sz", "o_cin", "o_act", "o_out", "o_dpre", "o_dout", "o_xin", "o_gan", "o_part", "o_dcin",
                                      "total")]


class AdamTensor(ctypes.Structure):
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("max_exp_avg_sq", c_void_p),
                ("numel", c_int64)]


class DecCfg(ctypes.Structure):
    _fields_ = [("channel_factor", c_int32), ("z_dim", c_int32), ("upsample_s", c_int32 * 2),
                ("upsample_t", c_int32 * 2), ("spectral_norm", c_int32), ("mma", c_int32)]


class FramesCfg(ctypes.Structure):
    _fields_ = [("n", c_int32), ("t", c_int32), ("h", c_int32), ("w", c_int32), ("n_stride", c_int64), ("k", c_int32), ("layout", c_int32),
                ("dst_row_bytes", c_int64), ("dst_frame_bytes", c_int64), ("dst_bytes", c_int64), ("row0", c_int32), ("col0", c_int32)]


class Enc3dCfg(ctypes.Structure):
    _fields_ = [("z_dim", c_int32), ("channels", c_int32 * 5), ("stride_s", c_int32 * 4), ("stride_t", c_int32 * 4),
                ("use_max_pool", c_int32)]


class VGGLayer(ctypes.Structure):
    _fields_ = [("h", c_int32), ("w", c_int32), ("cout", c_int32), ("tap", c_int32), ("offset", c_int64)]


class PatchDiscCfg(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("in_channels", "ndf", "n_layers", "use_actnorm", "spectral_norm")]


class Disc3DCfg(ctypes.Structure):
    _fields_ = [("res_type", c_int32), ("channels", c_int32 * 5), ("stride_s", c_int32 * 4), ("stride_t", c_int32 * 4), ("use_max_pool", c_int32),
                ("spectral_norm", c_int32)]


class Enc3dTrainCfg(ctypes.Structure):
    _fields_ = [("z_dim", c_int32), ("channels", c_int32 * 5), ("stride_s", c_int32 * 4), ("stride_t", c_int32 * 4), ("use_max_pool", c_int32)]


_lib = None

# symbol -> (restype, argtypes); also the list the CPU test-suite checks the .so exports
SYMBOLS = {
    "i2v_last_error": (c_char_p, []),
    "i2v_version": (c_int32, []),
    "i2v_device_count": (c_int32, []),
    "i2v_flow_create": (c_int32, [POINTER(FlowCfg), POINTER(c_void_p)]),
    "i2v_flow_destroy": (None, [c_void_p]),
    "i2v_flow_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_flow_workspace_bytes": (c_size_t, [c_void_p, c_int32]),
    "i2v_flow_param_bytes": (c_size_t, [c_void_p]),
    "i2v_flow_plan": (c_int32, [c_void_p, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "i2v_flow_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_flow_inverse": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_flow_train_create": (c_int32, [POINTER(FlowCfg), POINTER(c_void_p)]),
    "i2v_flow_train_destroy": (None, [c_void_p]),
    "i2v_flow_train_bind": (c_int32, [c_void_p, POINTER(_Tensor), POINTER(_Tensor), c_int32]),
    "i2v_flow_train_saved_bytes": (c_size_t, [c_void_p, c_int32]),
    "i2v_flow_train_saved_layout": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(FlowTrainLayout)]),
    "i2v_flow_train_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_flow_train_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                          c_void_p]),
    "i2v_adam_chunk": (c_int32, []),
    "i2v_adam_step": (c_int32, [c_void_p, c_void_p, c_int32, c_float, c_float, c_float, c_float, c_float, c_int32, c_int64, c_void_p]),
    "i2v_mlp_create": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_mlp_destroy": (None, [c_void_p]),
    "i2v_mlp_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_mlp_workspace_bytes": (c_size_t, [c_void_p, c_int32]),
    "i2v_mlp_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_channel_op": (c_int32, [c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_float, c_void_p]),
    "i2v_row_mean_std": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "i2v_actnorm_logdet": (c_int32, [c_void_p, c_int32, c_float, c_void_p, c_int32, c_void_p]),
    "i2v_probe_mfma_f16": (c_int32, [c_int32, c_int32, c_void_p, POINTER(c_double), c_void_p]),
    "i2v_gblock_create": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_gblock_destroy": (None, [c_void_p]),
    "i2v_gblock_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_gblock_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_gblock_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_size_t,
                                     c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "i2v_gblock_status": (c_int32, [c_void_p, POINTER(c_int32), c_int32, c_void_p]),
    "i2v_gblock_norm": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_int32,
                                  c_int32, c_int32, c_int32, c_void_p]),
    "i2v_embedder_create": (c_int32, [c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_embedder_destroy": (None, [c_void_p]),
    "i2v_embedder_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_embedder_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_embedder_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_encoder3d_create": (c_int32, [POINTER(Enc3dCfg), POINTER(c_void_p)]),
    "i2v_encoder3d_destroy": (None, [c_void_p]),
    "i2v_encoder3d_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_encoder3d_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_encoder3d_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_i3d_create": (c_int32, [c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_i3d_destroy": (None, [c_void_p]),
    "i2v_i3d_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_i3d_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_i3d_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_i3d_input_stage": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_fvd_stats_update": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "i2v_dti3d_create": (c_int32, [c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_i3d_features_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_i3d_feature_steps": (c_int32, [c_void_p, c_int32]),
    "i2v_i3d_features": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "i2v_diversity_update": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_i3d_unit_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "i2v_i3d_unit_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_size_t,
                                       c_void_p]),
    "i2v_i3d_mixed_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_i3d_mixed_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_i3d_maxpool_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "i2v_i3d_maxpool_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                          c_size_t, c_void_p]),
    "i2v_i3d_head_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32]),
    "i2v_i3d_head_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_vgg_create": (c_int32, [POINTER(c_void_p)]),
    "i2v_vgg_destroy": (None, [c_void_p]),
    "i2v_vgg_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_vgg_lin": (c_void_p, [c_void_p, c_int32]),
    "i2v_vgg_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_vgg_input_stage": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_vgg_features": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "i2v_vgg_conv_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_vgg_maxpool2": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_vgg_reduce_workspace_bytes": (c_size_t, [c_int32]),
    "i2v_lpips_layer": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_vgg_pairdiff_update": (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_vgg_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_vgg_backward_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_vgg_saved_layout": (c_int32, [c_int32, c_int32, c_int32, POINTER(VGGLayer)]),
    "i2v_vgg_features_saved": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_size_t, c_void_p]),
    "i2v_lpips_layer_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "i2v_vgg_backward": (c_int32, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_size_t, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                   c_void_p, c_size_t, c_void_p]),
    "i2v_vgg_dgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                     c_void_p]),
    "i2v_vgg_maxpool2_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_inception_create": (c_int32, [POINTER(c_void_p)]),
    "i2v_inception_destroy": (None, [c_void_p]),
    "i2v_inception_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_inception_block_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "i2v_inception_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_inception_input_stage": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_inception_features": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                         c_void_p]),
    "i2v_inception_conv_unit": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_size_t, c_void_p]),
    "i2v_inception_pool": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_size_t, c_void_p]),
    "i2v_inception_global_avg": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_inception_mixed_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "i2v_inception_mixed_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_inception_mixed_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_dec_create": (c_int32, [POINTER(DecCfg), POINTER(c_void_p)]),
    "i2v_dec_destroy": (None, [c_void_p]),
    "i2v_dec_load": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_dec_out_shape": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "i2v_dec_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_dec_flops_per_sample": (c_double, [c_void_p, c_int32, c_int32]),
    "i2v_dec_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_dec_forward_strided": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_size_t,
                                          c_int32, c_void_p]),
    "i2v_dec_prepare": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_int32, c_void_p]),
    "i2v_dec_prepare_cancel": (c_int32, [c_void_p]),
    "i2v_dec_workspace_bytes_realizations": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_dec_forward_realizations": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int64,
                                               c_void_p, c_size_t, c_void_p]),
    "i2v_dec_prepare_realizations": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_dec_join": (c_int32, [c_void_p, c_void_p]),
    "i2v_dec_set_side_stream": (c_int32, [c_void_p, c_void_p]),
    "i2v_dec_fallback_layers": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "i2v_dec_set_profile": (c_int32, [c_void_p, c_int32]),
    "i2v_dec_debug_tap": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_size_t]),
    "i2v_dec_get_spade_form": (c_int32, [c_void_p, c_int32, POINTER(c_int32)]),
    "i2v_conv_img_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                    POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_void_p]),
    "i2v_pointwise_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32,
                                     c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_void_p]),
    "i2v_dec_get_profile": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "i2v_dec_status": (c_int32, [c_void_p, POINTER(c_int32), c_int32, c_void_p]),
    "i2v_dec_get_layer_profile": (c_int32, [c_void_p, c_int32, ctypes.c_char_p, c_int32, POINTER(c_double), POINTER(c_double),
                                            POINTER(c_double), POINTER(c_int64), POINTER(c_int32)]),
    "i2v_frames_peak": (c_int32, [c_void_p, POINTER(FramesCfg), c_void_p, c_int32, c_void_p]),
    "i2v_frames_to_u8": (c_int32, [c_void_p, POINTER(FramesCfg), c_void_p, c_void_p, c_int32, c_void_p]),
    "i2v_recon_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_recon_range": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "i2v_recon_stats": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p, c_double, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_kl_normal": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
}

# The entries of include/i2v_hip_disc.h (the patch discriminator of stage-1 training), a table of its own: SYMBOLS is the list of
# include/i2v_hip.h, one to one.
DISC_SYMBOLS = {
    "i2v_patchdisc_create": (c_int32, [POINTER(PatchDiscCfg), POINTER(c_void_p)]),
    "i2v_patchdisc_destroy": (None, [c_void_p]),
    "i2v_patchdisc_bind": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_patchdisc_bind_grads": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_patchdisc_out_shape": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "i2v_patchdisc_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_patchdisc_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32]),
    "i2v_patchdisc_saved_layout": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                             POINTER(c_int64), POINTER(c_int64)]),
    "i2v_patchdisc_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                        c_void_p]),
    "i2v_patchdisc_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p,
                                         c_size_t, c_void_p]),
    "i2v_patchdisc_hinge": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "i2v_patchdisc_wgrad_plan": (c_int32, [c_int32, c_int32, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "i2v_patchdisc_unit_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_patchdisc_conv_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_patchdisc_dgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                           c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_patchdisc_wgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                           c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_patchdisc_head_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_patchdisc_power_iteration_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_patchdisc_actnorm_init_unit": (c_int32, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
}

# The entries of include/i2v_hip_disc3d.h (the temporal discriminator of stage-1 training), one to one.
_PP = POINTER(c_void_p)
DISC3D_SYMBOLS = {
    "i2v_disc3d_create": (c_int32, [POINTER(Disc3DCfg), POINTER(c_void_p)]),
    "i2v_disc3d_destroy": (None, [c_void_p]),
    "i2v_disc3d_bind": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_disc3d_bind_grads": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_disc3d_out_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "i2v_disc3d_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_disc3d_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_disc3d_saved_layout": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                          POINTER(c_int32), POINTER(c_int64)]),
    "i2v_disc3d_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, _PP, c_void_p, c_size_t, c_void_p,
                                     c_size_t, c_void_p]),
    "i2v_disc3d_backward": (c_int32, [c_void_p, c_void_p, _PP, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                      c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_fmap_loss_workspace_bytes": (c_size_t, []),
    "i2v_disc3d_fmap_loss": (c_int32, [_PP, _PP, POINTER(c_int64), c_int32, c_int32, c_float, c_void_p, _PP, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_sumsq": (c_int32, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "i2v_disc3d_wgrad_plan": (c_int32, [c_int32, c_int32, c_int32, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "i2v_disc3d_unit_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_disc3d_conv_unit": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_dgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_int32, c_int32, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_wgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                        c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_groupnorm_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "i2v_disc3d_groupnorm_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    "i2v_disc3d_groupnorm_backward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p,
                                                     c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_maxpool_unit": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "i2v_disc3d_maxpool_backward_unit": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_disc3d_head_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# The entries of include/i2v_hip_disc3d_gp.h (the temporal discriminator's gradient penalty with its gradient), one to one.
DISC3D_GP_SYMBOLS = {
    "i2v_disc3d_gp_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_disc3d_gp_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_disc3d_gp_saved_layout": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                             POINTER(c_int32), POINTER(c_int64)]),
    "i2v_disc3d_gp_backward": (c_int32, [c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t, c_void_p,
                                         c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_gp_backward_dev": (c_int32, [c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p, c_size_t,
                                             c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_gp_groupnorm_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "i2v_disc3d_gp_groupnorm_tangent_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p,
                                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_disc3d_gp_groupnorm_dual_backward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                                             c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
                                                             c_void_p]),
    "i2v_disc3d_gp_maxpool_tangent_unit": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_disc3d_gp_head_dual_unit": (c_int32, [c_void_p, c_void_p, c_float, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# The entries of include/i2v_hip_enc3d_train.h (the training path of the motion encoder), one to one.
ENC3D_TRAIN_SYMBOLS = {
    "i2v_enc3d_train_create": (c_int32, [POINTER(Enc3dTrainCfg), POINTER(c_void_p)]),
    "i2v_enc3d_train_destroy": (None, [c_void_p]),
    "i2v_enc3d_train_bind": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_enc3d_train_bind_grads": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_enc3d_train_out_shape": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "i2v_enc3d_train_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_enc3d_train_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32]),
    "i2v_enc3d_train_saved_layout": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                               POINTER(c_int32), POINTER(c_int64)]),
    "i2v_enc3d_train_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "i2v_enc3d_train_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_enc3d_kl_backward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p]),
    "i2v_enc3d_head_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "i2v_enc3d_head_forward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_enc3d_head_backward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                               c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
                                               c_void_p]),
}

# The entries of include/i2v_hip_gblock_train.h (the training path of one GeneratorBlock), one to one.
GBLOCK_TRAIN_SYMBOLS = {
    "i2v_gblock_train_create": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_gblock_train_destroy": (None, [c_void_p]),
    "i2v_gblock_train_bind": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_gblock_train_bind_grads": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_gblock_train_saved_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_gblock_train_workspace_bytes": (c_size_t, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_gblock_train_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "i2v_gblock_train_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                            c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_gblock_train_unit_workspace_bytes": (c_size_t, [c_int32, c_int64, c_int32]),
    "i2v_gblock_train_modnorm_backward_unit": (c_int32, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_gblock_train_pointwise_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_gblock_train_pointwise_wgrad_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_gblock_train_bias_grad_unit": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "i2v_gblock_train_linear_backward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                                        c_void_p]),
    "i2v_gblock_train_conv2d_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_size_t, c_void_p]),
}


# The entries of include/i2v_hip_gen_train.h (the training path of the Generator around its blocks: fc, up-sampling, image head), one to one.
GEN_TRAIN_SYMBOLS = {
    "i2v_gen_train_create": (c_int32, [c_int32, c_int32, POINTER(c_void_p)]),
    "i2v_gen_train_destroy": (None, [c_void_p]),
    "i2v_gen_train_bind": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_gen_train_bind_grads": (c_int32, [c_void_p, POINTER(_Tensor), c_int32]),
    "i2v_gen_train_fc_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "i2v_gen_train_head_saved_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_gen_train_head_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "i2v_gen_train_fc_slices": (c_int32, [c_int32]),
    "i2v_gen_train_fc_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "i2v_gen_train_fc_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "i2v_gen_train_head_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p,
                                             c_size_t, c_void_p]),
    "i2v_gen_train_head_backward": (c_int32, [c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                              c_void_p, c_size_t, c_void_p]),
    "i2v_gen_train_upsample_forward": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_gen_train_upsample_backward": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_gen_train_fc_forward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "i2v_gen_train_fc_backward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_size_t, c_void_p]),
    "i2v_gen_train_head_forward_unit": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                  c_size_t, c_void_p, c_size_t, c_void_p]),
    "i2v_gen_train_head_backward_unit": (c_int32, [c_void_p, c_void_p, c_size_t, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


def build(force=False):
    """Compile ``libi2v_hip.so`` for gfx950 in-tree (``make`` in csrc/; hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True)
    if not os.path.exists(LIB_PATH):
        raise I2VError(f"build did not produce {LIB_PATH}")
    return LIB_PATH


MEASURE_LIB_PATH = os.path.join(_PKG, "lib", "libi2v_hip_measure.so")


def build_measure():
    """Compile the MEASUREMENT build of the library (``make measure``: -DI2V_MEASURE, the F(4,3) kernel's structure switches).
    Only tests and A/B runs load it, through ``I2V_LIB_PATH`` in a process of their own."""
    subprocess.run(["make", "-C", CSRC, "-j4", "measure"], check=True)
    if not os.path.exists(MEASURE_LIB_PATH):
        raise I2VError(f"build did not produce {MEASURE_LIB_PATH}")
    return MEASURE_LIB_PATH


def lib():
    """The loaded shared library.  Fails loudly when it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise I2VError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"or `make -C {CSRC}`; this package has no CPU/eager fallback")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SYMBOLS.items()) + list(DISC_SYMBOLS.items()) + list(DISC3D_SYMBOLS.items()) + list(ENC3D_TRAIN_SYMBOLS.items())
                                 + list(GBLOCK_TRAIN_SYMBOLS.items()) + list(GEN_TRAIN_SYMBOLS.items()) + list(DISC3D_GP_SYMBOLS.items())):
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        raise I2VError(f"{what} failed ({rc}): {lib().i2v_last_error().decode(errors='replace')}")


def _require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise I2VError("libi2v_hip kernels need tensors on a HIP device (got a CPU tensor); "
                           "this package has no CPU fallback -- move the module and its inputs to 'cuda'")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise I2VError(f"expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")


def _call(name, *args):
    """One status-returning entry of the library; a non-zero code raises I2VError with the library's message."""
    _check(getattr(lib(), name)(*args), name)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_of(device):
    """torch.device of a handle: an explicit cuda device, else the current one.  A handle owns packed weights on ONE GPU."""
    if device is None:
        if not torch.cuda.is_available():
            raise I2VError("libi2v_hip needs a HIP device (torch.cuda.is_available() is False); this package has no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise I2VError(f"libi2v_hip kernels run on HIP devices only (got '{device}'); this package has no CPU fallback -- "
                       "move the module and its inputs to 'cuda'")
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


class _Workspace:
    """Caller-owned device scratch, cached per (device, size class) so its address is stable across calls."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


def _on_device(fn):
    """Method decorator of the native handles: reject tensors that live on another GPU, run with the handle's device current."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        tensors = [t for t in list(args) + list(kwargs.values()) if isinstance(t, torch.Tensor)]
        with self._on(*tensors):
            return fn(self, *args, **kwargs)
    return wrapper


class _Handle:
    """Common part of the native handles: the lifecycle (``<_PREFIX>_create`` / ``_load`` / ``_destroy``), the cached workspace and
    the device binding.  Creation, load and every call run with the handle's device current (``torch.cuda.device``), so the
    weights, the launches and the stream all belong to the GPU the tensors live on; tensors on another device are rejected (the
    C side checks the same thing and returns I2V_E_INVALID)."""
    _PREFIX = None   # "i2v_mlp", ...
    _h = None

    def _create(self, device, *args, symbol=None):
        """``<_PREFIX>_create(*args, &handle)`` (or ``symbol``) with ``device`` current."""
        h = c_void_p()
        with self._bind(device):
            _call(symbol or self._PREFIX + "_create", *args, ctypes.byref(h))
        self._h = h
        self._ws = _Workspace()

    def __del__(self):   # (the attributes -- a decoder's shared side stream, which its destroy synchronises -- are released after this)
        if self._h and _lib is not None:
            getattr(_lib, self._PREFIX + "_destroy")(self._h)
            self._h = None

    @_on_device
    def load(self, state_dict):
        """``<_PREFIX>_load``.  A load that fails leaves the handle unloaded: its next forward raises (I2V_E_STATE)."""
        arr, keep = _pack_state_dict(state_dict)
        _call(self._PREFIX + "_load", self._h, arr, len(arr))
        del keep

    def _scratch(self, nbytes, device, ws=None):
        """(pointer, size) of the handle's cached workspace (``ws``: another cache than ``_ws``), grown to ``nbytes``: the two
        arguments every forward passes as ``*ws``."""
        buf = (ws or self._ws).get(nbytes, device)
        return buf.data_ptr(), buf.numel()

    def _bind(self, device):
        self.device = _device_of(device)
        return torch.cuda.device(self.device)

    def _on(self, *tensors):
        for t in tensors:
            if t is not None and t.is_cuda and t.device != self.device:
                raise I2VError(f"tensor on {t.device} passed to a handle that lives on {self.device}: a native handle serves one GPU "
                               "(move the module with .to(device) -- that rebuilds the handle -- or the input)")
        return torch.cuda.device(self.device)


def _pack_state_dict(sd):
    """{key: tensor/ndarray} -> (ctypes array of i2v_tensor, keep-alive list)."""
    keep, items = [], []
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().contiguous().numpy()
        a = np.ascontiguousarray(v)
        if a.dtype == np.float32:
            dt = I2V_F32
        elif a.dtype == np.int64:
            dt = I2V_I64
        elif a.dtype == np.uint8:
            dt = I2V_U8
        else:
            raise I2VError(f"state_dict entry {k}: unsupported dtype {a.dtype}")
        kb = k.encode()
        keep.append((kb, a))
        items.append(_Tensor(kb, a.ctypes.data_as(c_void_p), a.size, dt))
    arr = (_Tensor * len(items))(*items)
    return arr, keep


class NativeFlow(_Handle):
    """Handle for ``i2v_flow_*`` (ConditionalFlow, flow_blocks.py:8-60)."""
    _PREFIX = "i2v_flow"

    def __init__(self, in_channels, embedding_dim, hidden_dim, hidden_depth, n_flows, control=False,
                 activation="lrelu", skip_actnorm=False, skip_shuffle=False, use_graph=True, device=None, linear_f16=None):
        self.linear_f16 = default_flow_f16() if linear_f16 is None else int(bool(linear_f16))
        cfg = FlowCfg(in_channels, embedding_dim, hidden_dim, hidden_depth, n_flows, int(control),
                      1 if activation == "lrelu" else 0, int(skip_actnorm), int(skip_shuffle), int(use_graph), self.linear_f16)
        self._create(device, ctypes.byref(cfg))
        self.embedding_dim = embedding_dim

    @property
    def param_bytes(self):
        return int(lib().i2v_flow_param_bytes(self._h))

    def plan(self, batch):
        """What a pass at ``batch`` launches on the loaded handle, asked of the launcher's own rule (host only, nothing runs):
        {"chain": "tile" | "generic", "kpw": k-blocks per wave, "ns": sample tiles per workgroup, "fold": bool}; kpw = ns = 0 and
        fold False on the generic chain."""
        v = [c_int32() for _ in range(4)]
        _call("i2v_flow_plan", self._h, int(batch), *(ctypes.byref(i) for i in v))
        chain, kpw, ns, fold = (i.value for i in v)
        return {"chain": "tile" if chain else "generic", "kpw": kpw, "ns": ns, "fold": bool(fold)}

    @_on_device
    def _run(self, x, embed, reverse):
        _require_gpu(x, embed)
        B = x.shape[0]
        if x.shape != (B, 64) or embed.shape != (B, self.embedding_dim):
            raise I2VError(f"flow: expected x [B,64] and embed [B,{self.embedding_dim}], got {tuple(x.shape)}, {tuple(embed.shape)}")
        nbytes = lib().i2v_flow_workspace_bytes(self._h, B)
        ws = self._scratch(nbytes, x.device)
        out = torch.empty_like(x)
        if reverse:
            _call("i2v_flow_inverse", self._h, x.data_ptr(), embed.data_ptr(), out.data_ptr(), *ws, B, _stream())
            return out
        logdet = torch.empty(B, dtype=torch.float32, device=x.device)
        _call("i2v_flow_forward", self._h, x.data_ptr(), embed.data_ptr(), out.data_ptr(), logdet.data_ptr(),
                                  *ws, B, _stream())
        return out, logdet

    @_on_device
    def forward(self, x, embed):
        return self._run(x, embed, False)

    def inverse(self, x, embed):
        return self._run(x, embed, True)


class NativeFlowTrain(_Handle):
    """Handle for ``i2v_flow_train_*``: the training path of ConditionalFlow (forward with saved activations, backward).  It packs
    nothing: ``bind`` hands over the DEVICE pointers of the module's own parameters, which the kernels read in place, so an
    optimiser step on them needs no re-load.  Gradients go either into bound tensors (``bind(..., grads=...)``) or into one flat
    buffer per backward call whose layout ``bind`` fixes (``flat_numel`` floats, ``flat_slices[name] = (offset, numel)``)."""
    _PREFIX = "i2v_flow_train"

    def __init__(self, in_channels, embedding_dim, hidden_dim, hidden_depth, n_flows, control=0, activation="lrelu",
                 skip_actnorm=False, skip_shuffle=False, device=None, linear_f16=0):
        cfg = FlowCfg(in_channels, embedding_dim, hidden_dim, hidden_depth, n_flows, int(control),
                      1 if activation == "lrelu" else 0, int(skip_actnorm), int(skip_shuffle), 0, int(bool(linear_f16)))
        self._create(device, ctypes.byref(cfg))
        self.embedding_dim = embedding_dim
        self._geometry = (hidden_dim, hidden_depth, embedding_dim, n_flows)
        self.flat_numel, self.flat_slices, self.bound_ptrs, self._keep = 0, {}, None, None

    def load(self, state_dict):
        raise I2VError("NativeFlowTrain packs nothing: bind() hands over the module's own parameters")

    @staticmethod
    def pointers(tensors):
        return tuple(t.data_ptr() for t in tensors.values())

    def bind(self, tensors, grads=None):
        """tensors: {state_dict key: device tensor} (float32 parameters, int64 Shuffle indices).  grads: {key: gradient tensor} of
        the float32 entries, or None for the flat layout (every gradient at a 16-byte aligned offset of one buffer)."""
        with self._on(*tensors.values()):
            items, gitems, keep, off = [], [], [], 0
            slices = {}
            for k, t in tensors.items():
                if not t.is_cuda or not t.is_contiguous():
                    raise I2VError(f"flow training: '{k}' must be a contiguous tensor on a HIP device (this package has no CPU fallback)")
                kb = k.encode()
                keep.append(kb)
                if t.dtype == torch.int64:
                    items.append(_Tensor(kb, t.data_ptr(), t.numel(), I2V_I64))
                    continue
                if t.dtype != torch.float32:
                    continue
                items.append(_Tensor(kb, t.data_ptr(), t.numel(), I2V_F32))
                if grads is None:
                    slices[k] = (off, t.numel())
                    gitems.append(_Tensor(kb, 4 * off, t.numel(), I2V_F32))
                    off += (t.numel() + 3) // 4 * 4
                else:
                    g = grads[k]
                    _require_gpu(g)
                    keep.append(g)
                    gitems.append(_Tensor(kb, g.data_ptr(), g.numel(), I2V_F32))
            n = len(items)
            gitems += [_Tensor(b"", None, 0, I2V_U8)] * (n - len(gitems))
            _call("i2v_flow_train_bind", self._h, (_Tensor * n)(*items), (_Tensor * n)(*gitems), n)
        self.flat_numel, self.flat_slices = (off, slices) if grads is None else (0, {})
        self.bound_ptrs = self.pointers(tensors)
        self._keep = (tensors, grads)

    def saved_layout(self, B):
        """{field: value} of ``i2v_flow_train_saved_layout`` at batch B: where each region of ``saved`` lies, in floats."""
        out = FlowTrainLayout()
        _call("i2v_flow_train_saved_layout", *self._geometry, B, ctypes.byref(out))
        return {n: int(getattr(out, n)) for n, _ in FlowTrainLayout._fields_}

    def forward(self, x, embed, saved=None):
        """-> (zt [B,64], logdet [B], saved): ``saved`` belongs to this pass and goes to ``backward``.  ``saved``: a uint8 device
        buffer of at least ``i2v_flow_train_saved_bytes`` to use instead of a fresh one (a test passes a pre-filled one)."""
        _require_gpu(x, embed)
        B = x.shape[0]
        if x.shape != (B, 64) or embed.shape != (B, self.embedding_dim):
            raise I2VError(f"flow: expected x [B,64] and embed [B,{self.embedding_dim}], got {tuple(x.shape)}, {tuple(embed.shape)}")
        with self._on(x, embed):
            if saved is None:
                saved = torch.empty(int(lib().i2v_flow_train_saved_bytes(self._h, B)), dtype=torch.uint8, device=x.device)
            elif saved.dtype != torch.uint8 or not saved.is_cuda or not saved.is_contiguous():
                raise I2VError("flow training: `saved` must be a contiguous uint8 tensor on a HIP device")
            zt = torch.empty_like(x)
            logdet = torch.empty(B, dtype=torch.float32, device=x.device)
            _call("i2v_flow_train_forward", self._h, x.data_ptr(), embed.data_ptr(), zt.data_ptr(), logdet.data_ptr(), saved.data_ptr(),
                                            saved.numel(), B, _stream())
        return zt, logdet, saved

    def backward(self, d_zt, d_logdet, saved, flat_grads=None, accumulate=False, need_dx=False, need_dembed=False):
        """Writes (accumulate: adds to) the parameter gradients -- into ``flat_grads`` (flat layout) or the bound gradient tensors --
        and returns (d_x or None, d_embed or None)."""
        _require_gpu(d_zt, d_logdet, flat_grads)
        B = d_zt.shape[0]
        if (flat_grads is None) != (self.flat_numel == 0) or (flat_grads is not None and flat_grads.numel() < self.flat_numel):
            raise I2VError("flow training: backward needs the flat gradient buffer exactly when bind() was given no gradient tensors")
        with self._on(d_zt, d_logdet, saved, flat_grads):
            dx = torch.empty(B, 64, dtype=torch.float32, device=d_zt.device) if need_dx else None
            de = torch.empty(B, self.embedding_dim, dtype=torch.float32, device=d_zt.device) if need_dembed else None
            _call("i2v_flow_train_backward", self._h, d_zt.data_ptr(), d_logdet.data_ptr(), saved.data_ptr(), saved.numel(),
                                             None if dx is None else dx.data_ptr(), None if de is None else de.data_ptr(),
                                             None if flat_grads is None else flat_grads.data_ptr(), int(bool(accumulate)), B, _stream())
        return dx, de


def adam_step(table, chunks, lr, beta1, beta2, eps, weight_decay, amsgrad, step):
    """One fused Adam launch over a device table of ``AdamTensor`` rows (uint8 tensor) and its chunk list (int32 [n, 2])."""
    with torch.cuda.device(table.device):
        _call("i2v_adam_step", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], lr, beta1, beta2, eps, weight_decay,
                               int(bool(amsgrad)), int(step), _stream())


def check_realizations(img, motion, z_dim, realizations):
    """Arguments of a decoder call with ``realizations`` = K samples per start frame: K an int >= 1, and -- for K > 1, where given --
    ``img`` [F,3,H,W] with ``motion`` [F*K, z_dim].  Raises I2VError before anything touches a device; returns K.  (K = 1 leaves the
    shapes to the plain forward's own checks.)"""
    if isinstance(realizations, bool) or not isinstance(realizations, int) or realizations < 1:
        raise I2VError(f"decoder: realizations must be an int >= 1, got {realizations!r}")
    K = realizations
    if K > 1 and img is not None:
        if img.dim() != 4 or img.shape[1] != 3 or motion.dim() != 2 or tuple(motion.shape) != (img.shape[0] * K, z_dim):
            raise I2VError(f"decoder: expected img [F,3,H,W] and motion [F*{K},{z_dim}] for {K} realizations, got {tuple(img.shape)}, "
                           f"{tuple(motion.shape)}")
    return K


class NativeDecoder(_Handle):
    """Handle for ``i2v_dec_*`` (Generator, decoder.py:55-120)."""
    _PREFIX = "i2v_dec"

    def __init__(self, channel_factor, z_dim, upsample_s, upsample_t, spectral_norm=True, mma=0, device=None):
        cfg = DecCfg(channel_factor, z_dim, (c_int32 * 2)(*upsample_s), (c_int32 * 2)(*upsample_t),
                     int(bool(spectral_norm)), mma)
        self._create(device, ctypes.byref(cfg))
        self.z_dim = z_dim
        t, hh, w = c_int32(), c_int32(), c_int32()
        _call("i2v_dec_out_shape", self._h, ctypes.byref(t), ctypes.byref(hh), ctypes.byref(w))
        self.out_shape = (t.value, hh.value, w.value)

    def flops_per_sample(self, img_h, img_w):
        return float(lib().i2v_dec_flops_per_sample(self._h, img_h, img_w))

    @_on_device
    def set_profile(self, on):
        _call("i2v_dec_set_profile", self._h, int(on))

    @_on_device
    def get_profile(self):
        a, b, e, c = c_double(), c_double(), c_double(), c_int64()
        _call("i2v_dec_get_profile", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(e), ctypes.byref(c))
        return {"conv3_ms": a.value, "conv3_flops": b.value, "conv3_mfma_flops": e.value, "conv3_launches": c.value}

    # i2v_dec_get_layer_profile's kernel code -> name
    KERNEL_NAMES = ("conv_mfma_f32", "conv_mfma_f16x3", "conv_wino_f16x3", "conv_wino4_f16x3", "conv_wino4g_f16x3", "conv_wino4_f32",
                    "conv_wino4_f16")

    @_on_device
    def get_layer_profile(self):
        """Per-layer totals of the profiled 3x3x3 conv launches since set_profile(True) (i2v_dec_get_layer_profile)."""
        rows = []
        for layer in range(12):
            name = ctypes.create_string_buffer(48)
            ms, fl, ex, n, k = c_double(), c_double(), c_double(), c_int64(), c_int32()
            _call("i2v_dec_get_layer_profile", self._h, layer, name, 48, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(ex),
                                               ctypes.byref(n), ctypes.byref(k))
            if n.value:
                rows.append({"layer": name.value.decode(), "kernel": self.KERNEL_NAMES[k.value],
                             "launches": int(n.value), "ms": ms.value, "flops": fl.value, "mfma_flops": ex.value})
        return rows

    @_on_device
    def status(self, reset=False):
        """Range guard of the split-fp16 operand format (i2v_dec_status): synchronises the current stream and returns the
        sticky flag word (bit 0: an activation left the fp16 range, the outputs since then are invalid)."""
        flags = c_int32()
        _call("i2v_dec_status", self._h, ctypes.byref(flags), int(bool(reset)), _stream())
        return int(flags.value)

    LAYER_NAMES = tuple(f"{b}.conv_{i}" for b in ("head_0", "g_0", "g_1", "g_2", "g_3", "g_4") for i in (0, 1))

    def fallback_layers(self):
        """mma = auto (i2v_dec_fallback_layers): the 3x3x3 convs the range guard has switched to the exact-fp32 kernels so far, as
        ``{"layers": [names], "whole_handle": bool, "reruns": n}``.  Empty for a checkpoint inside the split format's window."""
        mask, reruns = c_int32(), c_int32()
        _call("i2v_dec_fallback_layers", self._h, ctypes.byref(mask), ctypes.byref(reruns))
        return {"layers": [n for i, n in enumerate(self.LAYER_NAMES) if mask.value >> i & 1], "whole_handle": bool(mask.value >> 30 & 1),
                "reruns": int(reruns.value)}

    @_on_device
    def debug_tap(self, block, which, dst):
        """Test hook (i2v_dec_debug_tap): dst = float32 CUDA tensor or None."""
        if dst is None:
            _call("i2v_dec_debug_tap", self._h, -1, -1, None, 0)
        else:
            _call("i2v_dec_debug_tap", self._h, block, which, dst.data_ptr(), dst.numel())

    SPADE_FORMS = ("f43", "f23", "hl16", "f32")   # i2v_dec_get_spade_form's codes: the gamma | beta conv's kernel (dec_units_common names)

    def spade_forms(self):
        """The form SPADE's branch of each block took in the last forward (i2v_dec_get_spade_form); None: not run yet."""
        out = []
        for k in range(6):
            f = c_int32(-1)
            _call("i2v_dec_get_spade_form", self._h, k, ctypes.byref(f))
            out.append(self.SPADE_FORMS[f.value] if f.value >= 0 else None)
        return out

    def debug_tap_f64(self, block, which, pairs, device):
        """A NaN-filled float64 CUDA tensor [pairs, 2] set as the destination of one of the fp64 taps (6, 7, 8: (sum, sumsq) pairs, which
        the hook copies as bytes); read it after the next forward."""
        dst = torch.full((pairs, 2), float("nan"), dtype=torch.float64, device=device)
        self.debug_tap(block, which, dst.view(torch.float32).view(-1))
        return dst

    @_on_device
    def set_side_stream(self, stream):
        """i2v_dec_set_side_stream: run the handle's side work (SPADE branches, learned shortcuts, ``prepare``) on ``stream`` (a
        ``torch.cuda.Stream``, e.g. ``LatentPrefetcher.stream``) instead of a stream of the handle's own; ``None`` restores that.
        The binding keeps the stream object alive for as long as the handle uses it."""
        if stream is not None and stream.device != self.device:
            raise I2VError(f"side stream on {stream.device} for a handle on {self.device}")
        _call("i2v_dec_set_side_stream", self._h, c_void_p(stream.cuda_stream) if stream is not None else None)
        self._side_stream = stream
        self._prep = None

    def _scratch(self, nbytes, device):
        """The handle's workspace; before it is REPLACED by a larger one, the current stream joins the handle's side stream (a forked
        prepare may still be writing the old buffer: i2v_dec_join), so the caching allocator's stream-ordered free is safe."""
        buf = self._ws.buf
        if buf is not None and (buf.numel() < nbytes or buf.device != device):
            _call("i2v_dec_join", self._h, _stream())
            self._prep = None
        return super()._scratch(nbytes, device)

    @staticmethod
    def _version(t):
        """Version counter of a tensor, None for inference tensors (they do not track one: RuntimeError on access)."""
        try:
            return t._version
        except RuntimeError:
            return None

    def workspace_bytes(self, frames, img_h, img_w, realizations=1):
        """Workspace of a forward on ``frames`` start frames with ``realizations`` samples each (i2v_dec_workspace_bytes_realizations)."""
        return int(lib().i2v_dec_workspace_bytes_realizations(self._h, frames, check_realizations(None, None, None, realizations), img_h, img_w))

    @_on_device
    def prepare(self, img, realizations=1):
        """i2v_dec_prepare: enqueue the SPADE branches of all six blocks (they depend on the start frame only) on the HANDLE's side
        stream, ordered behind everything already on the current stream; the next ``forward`` with the SAME tensor (same storage,
        batch, size) waits for them per level instead of computing them.  The current stream stays free (e.g. for the cINN pass).
        Inference tensors (``torch.inference_mode``) carry no version counter, so an in-place refill between the prepare and its
        forward could not be detected: for them this is a no-op and the forward computes the branches itself (same bits).
        ``realizations``: the prepare serves ``forward(img, motion, realizations=K)`` with the same K (i2v_dec_prepare_realizations)."""
        # every check BEFORE any state changes: a raise must leave the Python side and the C side agreeing (nothing prepared)
        if getattr(self, "_prep", None) is not None:
            self._prep = None
            _call("i2v_dec_prepare_cancel", self._h)
        K = check_realizations(None, None, None, realizations)
        _require_gpu(img)
        B = img.shape[0]
        if img.dim() != 4 or img.shape[1] != 3:
            raise I2VError(f"decoder: expected img [B,3,H,W], got {tuple(img.shape)}")
        ver = self._version(img)
        if ver is None:
            return
        if K == 1:
            nbytes = lib().i2v_dec_workspace_bytes(self._h, B, img.shape[2], img.shape[3])
            ws = self._scratch(nbytes, img.device)
            _call("i2v_dec_prepare", self._h, img.data_ptr(), img.shape[2], img.shape[3], *ws, B, _stream())
        else:
            nbytes = lib().i2v_dec_workspace_bytes_realizations(self._h, B, K, img.shape[2], img.shape[3])
            ws = self._scratch(nbytes, img.device)
            _call("i2v_dec_prepare_realizations", self._h, img.data_ptr(), img.shape[2], img.shape[3], B, K, *ws,
                                                  _stream())
        # the C side recognises the prepared frames by ADDRESS; a caching allocator hands the same address to the next same-size
        # tensor and a buffer refilled in place keeps it, so the binding also remembers WHICH tensor (weak) and its version
        self._prep = (weakref.ref(img), ver)

    @staticmethod
    def _sample_strided(t, inner_shape):
        """(data_ptr, sample stride in floats) of a float32 tensor [B, *inner_shape] whose samples are contiguous blocks."""
        if t.dtype != torch.float32 or tuple(t.shape[1:]) != tuple(inner_shape):
            return None
        inner = 1
        for n, s in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
            if n != 1 and s != inner:
                return None
            inner *= n
        bs = t.stride(0) if t.shape[0] > 1 else inner
        return (t.data_ptr(), bs) if bs >= inner else None

    @_on_device
    def forward(self, img, motion, out=None, realizations=1):
        """i2v_dec_forward_strided.  ``img``: [B,3,H,W] whose samples are contiguous [3,H,W] blocks (any sample stride: e.g. the view
        ``seq[:, -1]`` of a [B,T,3,H,W] buffer).  ``out``: optional float32 view [B,T,3,H,W] with contiguous [T,3,H,W] sample blocks
        (e.g. ``buf[:, 16:32]`` of a [B,32,3,H,W] buffer) that receives the frames; a dense tensor is allocated otherwise.
        ``realizations`` = K > 1 (i2v_dec_forward_realizations): ``img`` holds F start frames, ``motion`` [F*K, z_dim] and ``out`` F*K
        samples, sample f*K + k = realization k of frame f -- the bits of ``forward(img.repeat_interleave(K, 0), motion)``, with the
        SPADE branches run once per frame."""
        K = check_realizations(img, motion, self.z_dim, realizations)
        for t in (img, motion):
            if not t.is_cuda:
                _require_gpu(t)   # raises: no CPU fallback
            if t.dtype != torch.float32:
                raise I2VError(f"expected float32 tensors, got {t.dtype}")
        prep, self._prep = getattr(self, "_prep", None), None
        if prep is not None and (prep[0]() is not img or prep[1] != self._version(img)):
            _call("i2v_dec_prepare_cancel", self._h)   # another tensor, or this one was written since
        Fr = img.shape[0]
        B = Fr * K
        if img.dim() != 4 or img.shape[1] != 3 or motion.shape != (B, self.z_dim):
            raise I2VError(f"decoder: expected img [B,3,H,W] and motion [B,{self.z_dim}], got {tuple(img.shape)}, {tuple(motion.shape)}")
        iv = self._sample_strided(img, img.shape[1:])
        if iv is None:
            img = img.contiguous()
            iv = (img.data_ptr(), 3 * img.shape[2] * img.shape[3])
        if not motion.is_contiguous():
            motion = motion.contiguous()
        if K == 1:
            nbytes = lib().i2v_dec_workspace_bytes(self._h, B, img.shape[2], img.shape[3])
        else:
            nbytes = lib().i2v_dec_workspace_bytes_realizations(self._h, Fr, K, img.shape[2], img.shape[3])
        ws = self._scratch(nbytes, img.device)
        T, H, W = self.out_shape
        if out is None:
            out = torch.empty(B, T, 3, H, W, dtype=torch.float32, device=img.device)
        ov = self._sample_strided(out, (T, 3, H, W)) if (out.is_cuda and out.device == img.device and out.shape[0] == B) else None
        if ov is None:
            raise I2VError(f"decoder: out must be a float32 [B={B},{T},3,{H},{W}] view on {img.device} with contiguous sample blocks, "
                           f"got {tuple(out.shape)} strides {out.stride()}")
        if K == 1:
            _call("i2v_dec_forward_strided", self._h, iv[0], img.shape[2], img.shape[3], iv[1], motion.data_ptr(), ov[0], ov[1],
                                             *ws, B, _stream())
        else:
            _call("i2v_dec_forward_realizations", self._h, iv[0], img.shape[2], img.shape[3], iv[1], Fr, K, motion.data_ptr(), ov[0],
                                                  ov[1], *ws, _stream())
        return out


CONV_IMG_FORMS = ("mfma", "gemm", "valu", "generic")   # i2v_conv_img_unit's form codes 0 .. 3


def conv_img_unit(x_cl, weight, bias, form=None, out=None, info=None):
    """``i2v_conv_img_unit``: the decoder's conv_img + tanh on x_cl [B, T, H, W, C] channels-last (device) with host ``weight``
    [3, C, 3, 3, 3] / ``bias`` [3] -> frames [B, T, 3, H, W].  form: None = the choice of a split-fp16 decoder, or one of
    CONV_IMG_FORMS (refused with I2VError where the form does not support the geometry).  out: a [B, T, 3, H, W] view whose samples
    may lie further apart than dense (stride(0) >= T * 3 * H * W, the rest contiguous).  info (dict): receives form / tch / range_flag."""
    _require_gpu(x_cl)
    if x_cl.dim() != 5:
        raise I2VError(f"conv_img_unit: expected [B, T, H, W, C], got {tuple(x_cl.shape)}")
    B, T, H, W, C = x_cl.shape
    w = np.ascontiguousarray(weight.detach().cpu().numpy() if isinstance(weight, torch.Tensor) else weight, dtype=np.float32)
    b = np.ascontiguousarray(bias.detach().cpu().numpy() if isinstance(bias, torch.Tensor) else bias, dtype=np.float32)
    if w.shape != (3, C, 3, 3, 3) or b.shape != (3,):
        raise I2VError(f"conv_img_unit: expected weight [3, {C}, 3, 3, 3] and bias [3], got {w.shape} / {b.shape}")
    if form is not None and form not in CONV_IMG_FORMS:
        raise I2VError(f"conv_img_unit: form {form!r} (one of {CONV_IMG_FORMS} or None)")
    if out is None:
        out = torch.empty(B, T, 3, H, W, dtype=torch.float32, device=x_cl.device)
    if (out.dtype != torch.float32 or out.device != x_cl.device or tuple(out.shape) != (B, T, 3, H, W) or not out[0].is_contiguous()
            or (B > 1 and out.stride(0) < T * 3 * H * W)):
        raise I2VError("conv_img_unit: out must be a float32 [B, T, 3, H, W] view on the input's device with dense samples")
    bstride = out.stride(0) if B > 1 else 0
    used, tch, flag = c_int32(-1), c_int32(0), c_int32(0)
    with torch.cuda.device(x_cl.device):
        _call("i2v_conv_img_unit", x_cl.data_ptr(), w.ctypes.data_as(c_void_p), b.ctypes.data_as(c_void_p), B, T, H, W, C,
                                   -1 if form is None else CONV_IMG_FORMS.index(form), out.data_ptr(), bstride, ctypes.byref(used),
                                   ctypes.byref(tch), ctypes.byref(flag), _stream())
    if info is not None:
        info.update(form=CONV_IMG_FORMS[used.value], tch=tch.value, range_flag=flag.value)
    return out


def pointwise_unit(x, weight, bias=None, res=None, coef=None, rows_per_sample=None, lrelu=False, split16=True, transposed=False, info=None):
    """``i2v_pointwise_unit``: act((x * A + B) @ weight^T + bias + res) on x [M, Cin] (device) with host ``weight`` [Cout, Cin] and ``bias``
    [Cout]; coef [M / rows_per_sample, Cin, 2] = the (A, B) table (device).  split16: the split-fp16 GEMM, else the exact-fp32 one.
    transposed: the output as [Cout, M].  info (dict): receives tile_n / range_flag."""
    _require_gpu(x, res, coef)
    M, Cin = x.shape
    w = np.ascontiguousarray(weight.detach().cpu().numpy() if isinstance(weight, torch.Tensor) else weight, dtype=np.float32)
    if w.ndim != 2 or w.shape[1] != Cin:
        raise I2VError(f"pointwise_unit: expected weight [Cout, {Cin}], got {w.shape}")
    Cout = w.shape[0]
    b = None
    if bias is not None:
        b = np.ascontiguousarray(bias.detach().cpu().numpy() if isinstance(bias, torch.Tensor) else bias, dtype=np.float32)
        if b.shape != (Cout,):
            raise I2VError(f"pointwise_unit: expected bias [{Cout}], got {b.shape}")
    P = M if rows_per_sample is None else int(rows_per_sample)
    if res is not None and tuple(res.shape) != (M, Cout):
        raise I2VError(f"pointwise_unit: expected res [{M}, {Cout}], got {tuple(res.shape)}")
    if coef is not None and tuple(coef.shape) != ((M + P - 1) // P, Cin, 2):
        raise I2VError(f"pointwise_unit: expected coef [{(M + P - 1) // P}, {Cin}, 2], got {tuple(coef.shape)}")
    out = torch.empty((Cout, M) if transposed else (M, Cout), dtype=torch.float32, device=x.device)
    tile, flag = c_int32(0), c_int32(0)
    with torch.cuda.device(x.device):
        _call("i2v_pointwise_unit", x.data_ptr(), w.ctypes.data_as(c_void_p), None if b is None else b.ctypes.data_as(c_void_p),
                                    None if res is None else res.data_ptr(), None if coef is None else coef.data_ptr(), out.data_ptr(), M, P,
                                    Cin, Cout, int(bool(lrelu)), int(bool(split16)), int(bool(transposed)), ctypes.byref(tile),
                                    ctypes.byref(flag), _stream())
    if info is not None:
        info.update(tile_n=tile.value, range_flag=flag.value)
    return out


class NativeMLP(_Handle):
    """Handle for ``i2v_mlp_*`` (BasicFullyConnectedNet, modules.py:9-30)."""
    _PREFIX = "i2v_mlp"

    def __init__(self, dim, hidden_dim, depth, out_dim, device=None):
        self._create(device, dim, hidden_dim, depth, out_dim)
        self.dim, self.out_dim = dim, out_dim

    @_on_device
    def forward(self, x):
        _require_gpu(x)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise I2VError(f"mlp: expected x [B,{self.dim}], got {tuple(x.shape)}")
        B = x.shape[0]
        ws = self._scratch(lib().i2v_mlp_workspace_bytes(self._h, B), x.device)
        y = torch.empty(B, self.out_dim, dtype=torch.float32, device=x.device)
        _call("i2v_mlp_forward", self._h, x.data_ptr(), y.data_ptr(), *ws, B, _stream())
        return y


OP_ACTNORM_FWD, OP_ACTNORM_REV, OP_INVLRELU_FWD, OP_INVLRELU_REV, OP_GATHER = range(5)


def _channel_op(op, x, p0=None, p1=None, idx=None, alpha=0.0):
    _require_gpu(x)
    if x.dim() < 2:
        raise I2VError("channel op: need a [B, C, ...] tensor")
    B, C = x.shape[0], x.shape[1]
    inner = x.numel() // (B * C)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _call("i2v_channel_op", op, x.data_ptr(), out.data_ptr(), B, C, inner,
                                p0.data_ptr() if p0 is not None else None, p1.data_ptr() if p1 is not None else None,
                                idx.data_ptr() if idx is not None else None, float(alpha), _stream())
    return out


def actnorm(x, loc, scale, reverse):
    """ActNorm.forward / reverse arithmetic (modules.py:80,100) on [B,C,H,W]."""
    loc = loc.detach().reshape(-1).contiguous()
    scale = scale.detach().reshape(-1).contiguous()
    _require_gpu(loc, scale)
    return _channel_op(OP_ACTNORM_REV if reverse else OP_ACTNORM_FWD, x, loc, scale)


def actnorm_logdet(scale, hw, batch):
    scale = scale.detach().reshape(-1).contiguous()
    _require_gpu(scale)
    out = torch.empty(batch, dtype=torch.float32, device=scale.device)
    with torch.cuda.device(scale.device):
        _call("i2v_actnorm_logdet", scale.data_ptr(), scale.numel(), float(hw), out.data_ptr(), batch, _stream())
    return out


def probe_mfma_f16(device, workgroups=2048, iters=4096, reps=3):
    """Sustained fp16 matrix-core rate with live operands (TFLOP/s of v_mfma_f32_32x32x16_f16 actually executed by an
    MFMA-only loop of the conv kernel's shape; measurement helper for bench.py).  Median of ``reps`` event-timed launches
    after one warm-up launch of the same length (so the clock has settled)."""
    scratch = torch.empty(workgroups * 512, dtype=torch.float32, device=device)
    flops = c_double()
    rates = []
    with torch.cuda.device(scratch.device):
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _call("i2v_probe_mfma_f16", workgroups, iters, scratch.data_ptr(), ctypes.byref(flops), _stream())
            e1.record()
            e1.synchronize()
            if r:
                rates.append(flops.value / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    rates.sort()
    return rates[len(rates) // 2]


def inv_lrelu(x, alpha, reverse):
    return _channel_op(OP_INVLRELU_REV if reverse else OP_INVLRELU_FWD, x, alpha=alpha)


def gather_channels(x, idx):
    idx = idx.detach().contiguous()
    if not idx.is_cuda or idx.dtype != torch.int64:
        raise I2VError("gather_channels: idx must be an int64 tensor on the GPU")
    return _channel_op(OP_GATHER, x, idx=idx)


def channel_mean_std(flat):
    """flat [C, N] -> (mean [C], unbiased std [C])."""
    _require_gpu(flat)
    C, N = flat.shape
    mean = torch.empty(C, dtype=torch.float32, device=flat.device)
    std = torch.empty(C, dtype=torch.float32, device=flat.device)
    with torch.cuda.device(flat.device):
        _call("i2v_row_mean_std", flat.data_ptr(), C, N, mean.data_ptr(), std.data_ptr(), _stream())
    return mean, std


# ---------------------------------------------------------------------------------------------- output stage (csrc/i2v_frames.hip)
FRAMES_PEAK, FRAMES_UNIT = 0, 1
FRAMES_STRIP, FRAMES_CLIPS = 0, 1


def frames_geometry(x):
    """Host-side shape check of the output stage's input (before anything touches a device): ``x`` float32 ``[N, T, 3, H, W]`` or
    ``[F, K, T, 3, H, W]`` whose ``[T, 3, H, W]`` blocks are contiguous, with one element stride between the N (= F*K) samples -- a
    dense tensor, a ``[:, :16]`` view of a longer buffer, the ``[F, K, ...]`` view of ``Model.sample``.  Returns (n, k, t, h, w, n_stride)."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() not in (5, 6) or x.shape[-3] != 3 or x.numel() == 0:
        raise I2VError("frames: expected a non-empty float32 tensor [N,T,3,H,W] or [F,K,T,3,H,W], got "
                       + (f"{x.dtype} {tuple(x.shape)}" if torch.is_tensor(x) else repr(type(x))))
    k = x.shape[1] if x.dim() == 6 else 1
    t, _, h, w = x.shape[-4:]
    per, inner = t * 3 * h * w, 1
    for size, stride in zip(reversed(x.shape[-4:]), reversed(x.stride()[-4:])):
        if size != 1 and stride != inner:
            raise I2VError(f"frames: the [T,3,H,W] block of a sample must be contiguous (strides {x.stride()})")
        inner *= size
    if x.dim() == 6:
        f = x.shape[0]
        sk = x.stride(1) if k > 1 else per
        sf = x.stride(0) if f > 1 else sk * k
        if sk < per or sf != sk * k:
            raise I2VError(f"frames: [F,K,...] needs one stride between its F*K samples (strides {x.stride()})")
        return f * k, k, t, h, w, sk
    n = x.shape[0]
    ns = x.stride(0) if n > 1 else per
    if ns < per:
        raise I2VError(f"frames: samples overlap (sample stride {ns} < {per})")
    return n, 1, t, h, w, ns


def _frames_peak_cell(out, device):
    if out is None:
        return torch.empty(1, dtype=torch.float32, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.numel() != 1:
        raise I2VError("frames_peak: out must be a float32 tensor with one element")
    return out


def frames_peak(x, out=None, accumulate=False):
    """Maximum of all raw values of ``x`` (see ``frames_geometry``) into a one-element float32 DEVICE tensor (i2v_frames_peak; no host
    round trip).  ``accumulate`` keeps ``max(out, max x)``: one peak for a job converted batch by batch (needs ``out``)."""
    n, k, t, h, w, ns = frames_geometry(x)
    if accumulate and out is None:
        raise I2VError("frames_peak: accumulate=True needs the running peak in out")
    if out is not None:
        _frames_peak_cell(out, None)
    _require_gpu(out)
    if not x.is_cuda:
        raise I2VError("frames_peak: libi2v_hip kernels need tensors on a HIP device (got a CPU tensor); this package has no CPU fallback")
    out = _frames_peak_cell(out, x.device)
    cfg = FramesCfg(n=n, t=t, h=h, w=w, n_stride=ns, k=1)
    with torch.cuda.device(x.device):
        _call("i2v_frames_peak", x.data_ptr(), ctypes.byref(cfg), out.data_ptr(), int(bool(accumulate)), _stream())
    return out


def frames_to_u8(x, peak=None, out=None, mode="peak", layout="strip", row0=0, col0=0):
    """``x`` (see ``frames_geometry``) -> interleaved uint8 on the device (i2v_frames_to_u8).
    ``mode`` "peak": GIF semantics of ``convert_seq2gif`` / ``convert_grid2gif``, scaled by the device float ``peak`` of ``frames_peak``
    (None: the peak of ``x`` itself is taken first); "unit": ``trunc(clamp(denorm(x) * 255 + 0.5, 0, 255))``.
    ``layout`` "strip": ``[T, K*H, (N/K)*W, 3]`` (a 6-dim ``x`` is a grid: realization k in row k); ``out`` may be a larger contiguous
    uint8 ``[T, rows, cols, 3]`` tensor of which this call fills the block at pixel (``row0``, ``col0``).  "clips": ``[N, T, H, W, 3]``
    (``[F, K, T, H, W, 3]`` for a 6-dim ``x``).  Returns ``out``."""
    n, k, t, h, w, ns = frames_geometry(x)
    if mode not in ("peak", "unit"):
        raise I2VError(f"frames_to_u8: mode must be 'peak' or 'unit', got {mode!r}")
    if layout not in ("strip", "clips"):
        raise I2VError(f"frames_to_u8: layout must be 'strip' or 'clips', got {layout!r}")
    if mode == "unit" and peak is not None:
        raise I2VError("frames_to_u8: mode 'unit' takes no peak")
    if peak is not None:
        _frames_peak_cell(peak, None)
    for name, v in (("row0", row0), ("col0", col0)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise I2VError(f"frames_to_u8: {name} must be an int >= 0, got {v!r}")
    if layout == "clips":
        if row0 or col0:
            raise I2VError("frames_to_u8: the clip layout has no placement (row0 = col0 = 0)")
        shape = tuple(x.shape[:-4]) + (t, h, w, 3)
        if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise I2VError(f"frames_to_u8: out must be a contiguous uint8 tensor {shape}")
    else:
        shape = (t, k * h, (n // k) * w, 3)
        if out is not None:
            if out.dtype != torch.uint8 or out.dim() != 4 or out.shape[0] != t or out.shape[3] != 3 or not out.is_contiguous():
                raise I2VError(f"frames_to_u8: out must be a contiguous uint8 tensor [{t}, rows, cols, 3], got "
                               f"{out.dtype} {tuple(out.shape)}")
            if row0 + k * h > out.shape[1] or col0 + (n // k) * w > out.shape[2]:
                raise I2VError(f"frames_to_u8: the block [{k * h} x {(n // k) * w}] at ({row0}, {col0}) does not fit out {tuple(out.shape)}")
    if not x.is_cuda or (out is not None and out.device != x.device) or (peak is not None and peak.device != x.device):
        raise I2VError("frames_to_u8: libi2v_hip kernels need x, peak and out on one HIP device; this package has no CPU fallback")
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    if mode == "peak" and peak is None:
        peak = frames_peak(x)
    cfg = FramesCfg(n=n, t=t, h=h, w=w, n_stride=ns, k=k if layout == "strip" else 1, layout=FRAMES_STRIP if layout == "strip" else FRAMES_CLIPS,
                    dst_bytes=out.numel(), row0=row0, col0=col0)
    if layout == "strip":
        cfg.dst_row_bytes, cfg.dst_frame_bytes = out.shape[2] * 3, out.shape[1] * out.shape[2] * 3
    with torch.cuda.device(x.device):
        _call("i2v_frames_to_u8", x.data_ptr(), ctypes.byref(cfg), peak.data_ptr() if peak is not None else None, out.data_ptr(),
                                  FRAMES_PEAK if mode == "peak" else FRAMES_UNIT, _stream())
    return out


def default_flow_f16():
    """Operand precision of the cINN's Linear layers: 0 = exact fp32 matrix cores (default), 1 = fp16 operands with fp32
    accumulation (BASELINE configs[4]; i2v_flow_cfg.linear_f16); env I2V_FLOW_F16."""
    return int(os.environ.get("I2V_FLOW_F16", "0"))


def parse_mma(v):
    """0 / 1 / 2 / 3, "auto" (= 2) or "fp16" (= 3) -> the i2v_dec_cfg.mma value."""
    if isinstance(v, str):
        v = v.strip().lower()
        if v == "auto":
            return 2
        if v == "fp16":
            return 3
        return int(v)
    return int(v)


def default_mma():
    """Matrix-core mode of the 3x3x3 convolutions: 1 = split-fp16 (default), 0 = exact fp32 MFMA, 2 / "auto" = split-fp16 with the
    per-layer fallback to exact fp32 behind the range guard (every forward synchronises), 3 / "fp16" = opt-in half precision: the F(4,3)
    block convs on one-term fp16 operands (one MFMA per product); env I2V_DEC_MMA."""
    return parse_mma(os.environ.get("I2V_DEC_MMA", "1"))


class NativeGBlock(_Handle):
    """Handle for ``i2v_gblock_*`` (GeneratorBlock, decoder.py:7-52; tensors in the reference layout [B,C,T,H,W])."""
    _PREFIX = "i2v_gblock"

    def __init__(self, n_in, n_out, z_dim, spectral_norm=True, mma=None, device=None):
        mma = default_mma() if mma is None else parse_mma(mma)
        if mma == 2:   # auto: a stand-alone block has no re-run loop behind the range guard; it runs split-fp16 (status() reports)
            mma = 1
        self._create(device, n_in, n_out, z_dim, int(bool(spectral_norm)), mma)
        self.n_in, self.n_out, self.n_mid, self.z_dim = n_in, n_out, min(n_in, n_out), z_dim

    def _geom(self, x, channels):
        if x.dim() != 5 or x.shape[1] != channels:
            raise I2VError(f"expected x [B,{channels},T,H,W], got {tuple(x.shape)}")
        B, _, T, H, W = x.shape
        ws = self._scratch(lib().i2v_gblock_workspace_bytes(self._h, B, T, H, W), x.device)
        return B, T, H, W, ws

    @_on_device
    def forward(self, x, z, img):
        _require_gpu(x, z, img)
        B, T, H, W, ws = self._geom(x, self.n_in)
        if z.shape != (B, self.z_dim) or img.dim() != 4 or img.shape[:2] != (B, 3):
            raise I2VError(f"GeneratorBlock: expected z [B,{self.z_dim}] and img [B,3,h,w], got {tuple(z.shape)}, {tuple(img.shape)}")
        out = torch.empty(B, self.n_out, T, H, W, dtype=torch.float32, device=x.device)
        _call("i2v_gblock_forward", self._h, x.data_ptr(), z.data_ptr(), img.data_ptr(), img.shape[2], img.shape[3],
                                    out.data_ptr(), *ws, B, T, H, W, _stream())
        return out

    @_on_device
    def status(self, reset=False):
        """Range guard of this block's split-fp16 operand writers (i2v_gblock_status): synchronises, returns the flag word."""
        flags = c_int32()
        _call("i2v_gblock_status", self._h, ctypes.byref(flags), int(bool(reset)), _stream())
        return int(flags.value)

    @_on_device
    def norm(self, part, x, cond):
        _require_gpu(x, cond)
        B, T, H, W, ws = self._geom(x, self.n_mid if part == 1 else self.n_in)
        ih = iw = 0
        if part == 0:
            if cond is None or cond.dim() != 4 or cond.shape[:2] != (B, 3):
                raise I2VError("Spade: expected the start frame [B,3,h,w]")
            ih, iw = cond.shape[2], cond.shape[3]
        if part == 1 and (cond is None or cond.shape != (B, self.z_dim)):
            raise I2VError(f"ADAIN: expected z [B,{self.z_dim}]")
        out = torch.empty_like(x)
        _call("i2v_gblock_norm", self._h, part, x.data_ptr(), cond.data_ptr() if cond is not None else None, ih, iw,
                                 out.data_ptr(), *ws, B, T, H, W, _stream())
        return out


class NativeNorm:
    """A lone Spade / ADAIN / Norm3D (normalization_layer.py:5-51) on top of a partially loaded ``i2v_gblock``."""
    _PART = {"spade": (0, "norm_0."), "adain": (1, "norm_1."), "norm3d": (2, "norm_s.")}

    def __init__(self, kind, num_features, z_dim, mma=None, device=None):
        self.part, self.prefix = self._PART[kind]
        self.blk = NativeGBlock(num_features, num_features, z_dim if z_dim else 64, spectral_norm=False, mma=mma, device=device)

    def load(self, state_dict):
        self.blk.load({self.prefix + k: v for k, v in state_dict.items()})

    def forward(self, x, cond):
        return self.blk.norm(self.part, x, cond)


class NativeEmbedder(_Handle):
    """Handle for ``i2v_embedder_*`` (ResnetEncoder.encode(x).mode(), AE.py:91-166)."""
    _PREFIX = "i2v_embedder"

    def __init__(self, z_dim, use_batchnorm, device=None):
        self._create(device, z_dim, int(bool(use_batchnorm)))
        self.z_dim = z_dim

    @_on_device
    def forward(self, img):
        _require_gpu(img)
        if img.dim() != 4 or img.shape[1] != 3:
            raise I2VError(f"embedder: expected img [B,3,H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        ws = self._scratch(lib().i2v_embedder_workspace_bytes(self._h, B, H, W), img.device)
        out = torch.empty(B, self.z_dim, dtype=torch.float32, device=img.device)
        _call("i2v_embedder_forward", self._h, img.data_ptr(), H, W, out.data_ptr(), *ws, B, _stream())
        return out


class NativeEncoder3D(_Handle):
    """Handle for ``i2v_encoder3d_*`` (Encoder.forward, resnet3D.py:138-219)."""
    _PREFIX = "i2v_encoder3d"

    def __init__(self, z_dim, channels, stride_s, stride_t, device=None):
        cfg = Enc3dCfg(z_dim, (c_int32 * 5)(*channels), (c_int32 * 4)(*stride_s), (c_int32 * 4)(*stride_t), 0)
        self._create(device, ctypes.byref(cfg))
        self.z_dim = z_dim

    @_on_device
    def forward(self, x, eps=None):
        _require_gpu(x, eps)
        if x.dim() != 5 or x.shape[1] != 3:
            raise I2VError(f"encoder: expected x [B,3,T,H,W], got {tuple(x.shape)}")
        B, _, T, H, W = x.shape
        if eps is not None and tuple(eps.shape) != (B, self.z_dim):
            raise I2VError(f"encoder: expected eps [{B},{self.z_dim}], got {tuple(eps.shape)}")
        ws = self._scratch(lib().i2v_encoder3d_workspace_bytes(self._h, B, T, H, W), x.device)
        mu = torch.empty(B, self.z_dim, dtype=torch.float32, device=x.device)
        logvar = torch.empty_like(mu)
        sample = torch.empty_like(mu) if eps is not None else None
        _call("i2v_encoder3d_forward", self._h, x.data_ptr(), T, H, W, eps.data_ptr() if eps is not None else None,
                                       sample.data_ptr() if sample is not None else None, mu.data_ptr(), logvar.data_ptr(),
                                       *ws, B, _stream())
        return sample, mu, logvar


class NativeI3D(_Handle):
    """Handle for ``i2v_i3d_*`` (the Kinetics-400 I3D of metrics/PyTorch_FVD/I3D.py with FVD_logging.preprocess as its input stage) and,
    with ``dt_length`` 16 or 32, for the dynamic-texture I3D of metrics/DTFVD/ID3.py / ID3_32.py (``i2v_dti3d_create``)."""
    _PREFIX = "i2v_i3d"

    def __init__(self, num_classes, in_channels=3, device=None, dt_length=None):
        if dt_length is None:
            self._create(device, num_classes, in_channels)
        else:
            self._create(device, num_classes, dt_length, symbol="i2v_dti3d_create")
        self.num_classes = num_classes
        self.dt_length = dt_length

    @_on_device
    def forward(self, frames, denorm):
        """frames [B, T, 3, H, W] (the decoder's output layout), ``denorm``: the values are in [-1, 1] -> logits [B, num_classes]."""
        _require_gpu(frames)
        if frames.dim() != 5 or frames.shape[2] != 3:
            raise I2VError(f"i3d: expected frames [B,T,3,H,W], got {tuple(frames.shape)}")
        B, T, _, H, W = frames.shape
        nbytes = lib().i2v_i3d_workspace_bytes(self._h, B, T, H, W)
        if nbytes == 0:
            raise I2VError(f"i3d: no plan for frames {tuple(frames.shape)} (at least 9 frames of at least 2 x 2 pixels are needed)")
        ws = self._scratch(nbytes, frames.device)
        out = torch.empty(B, self.num_classes, dtype=torch.float32, device=frames.device)
        _call("i2v_i3d_forward", self._h, frames.data_ptr(), B, T, H, W, int(bool(denorm)), out.data_ptr(), *ws,
                                 _stream())
        return out

    @_on_device
    def features(self, frames, denorm=False, t_out=None):
        """``i2v_i3d_features``: frames [B, T_in, 3, H, W] -> the average pool's output [B, 1024, T'] (``get_representation``).  ``t_out``
        frames enter the network, frame t read from source frame t % T_in (None: T_in)."""
        _require_gpu(frames)
        if frames.dim() != 5 or frames.shape[2] != 3:
            raise I2VError(f"i3d: expected frames [B,T,3,H,W], got {tuple(frames.shape)}")
        B, T, _, H, W = frames.shape
        t_out = T if t_out is None else int(t_out)
        steps = lib().i2v_i3d_feature_steps(self._h, t_out)
        nbytes = lib().i2v_i3d_features_workspace_bytes(self._h, B, t_out, H, W) if steps > 0 else 0
        if nbytes == 0:
            need = 25 if self.dt_length == 32 else 9
            raise I2VError(f"i3d: no plan for frames {tuple(frames.shape)} with {t_out} frames per clip (at least {need} frames of at least "
                           "2 x 2 pixels are needed)")
        ws = self._scratch(nbytes, frames.device)
        out = torch.empty(B, 1024, steps, dtype=torch.float32, device=frames.device)
        _call("i2v_i3d_features", self._h, frames.data_ptr(), B, T, t_out, H, W, int(bool(denorm)), out.data_ptr(), *ws, _stream())
        return out

    # ---- sub-modules on channels-last tensors [B, T, H, W, C] (tests and inspection)
    UNIT_STEM, UNIT_2B, UNIT_2C, UNIT_MIXED, UNIT_HEAD = 0, 1, 2, 3, 57

    @staticmethod
    def _require_cl(x, what):
        _require_gpu(x)
        if x.dim() != 5 or x.dtype != torch.float32 or not x.is_contiguous():
            raise I2VError(f"{what}: expected a contiguous fp32 tensor [B,T,H,W,C], got {tuple(x.shape)} {x.dtype}")

    def unit_shape(self, unit, t, h, w):
        """``i2v_i3d_unit_shape``: (cin, cout, (To, Ho, Wo)) of conv unit ``unit`` on a [t, h, w] map."""
        cin, cout, od = c_int32(), c_int32(), (c_int32 * 3)()
        _call("i2v_i3d_unit_shape", self._h, unit, t, h, w, ctypes.byref(cin), ctypes.byref(cout), od)
        return cin.value, cout.value, tuple(od)

    @_on_device
    def unit_forward(self, unit, x, out=None, out_off=0):
        """``i2v_i3d_unit_forward``: x [B, T, H, W, in_cs] -> channels [out_off, out_off + cout) of ``out`` [B, To, Ho, Wo, out_cs] (a new
        tensor of cout channels when None)."""
        self._require_cl(x, "i3d unit")
        B, T, H, W, cs = x.shape
        _, cout, od = self.unit_shape(unit, T, H, W)
        if out is None:
            out = torch.empty(B, *od, cout, dtype=torch.float32, device=x.device)
        self._require_cl(out, "i3d unit")
        if tuple(out.shape[:4]) != (B, *od):
            raise I2VError(f"i3d unit: expected an output [{B},{od[0]},{od[1]},{od[2]},C], got {tuple(out.shape)}")
        _call("i2v_i3d_unit_forward", self._h, unit, x.data_ptr(), B, T, H, W, cs, out.data_ptr(), out.shape[4], out_off, out.numel(),
                                      _stream())
        return out

    @_on_device
    def mixed_forward(self, block, x):
        """``i2v_i3d_mixed_forward``: Mixed block ``block`` (0 = 3b .. 8 = 5c) on x [B, T, H, W, cin] -> [B, T, H, W, Co]."""
        self._require_cl(x, "i3d mixed")
        B, T, H, W, cs = x.shape
        cin = self.unit_shape(self.UNIT_MIXED + 6 * block, T, H, W)[0]
        if cs != cin:
            raise I2VError(f"i3d mixed: block {block} reads {cin} channels, got {cs}")
        co = sum(self.unit_shape(self.UNIT_MIXED + 6 * block + j, T, H, W)[1] for j in (0, 2, 4, 5))
        ws = self._scratch(lib().i2v_i3d_mixed_workspace_bytes(self._h, block, B, T, H, W), x.device)
        out = torch.empty(B, T, H, W, co, dtype=torch.float32, device=x.device)
        _call("i2v_i3d_mixed_forward", self._h, block, x.data_ptr(), B, T, H, W, out.data_ptr(), *ws, _stream())
        return out

    def maxpool_shape(self, kernel, stride, t, h, w):
        """``i2v_i3d_maxpool_shape``: (To, Ho, Wo) of the max pool (kT, k, k) / (sT, s, s) on a [t, h, w] map."""
        od = (c_int32 * 3)()
        _call("i2v_i3d_maxpool_shape", self._h, kernel[0], kernel[1], stride[0], stride[1], t, h, w, od)
        return tuple(od)

    @_on_device
    def maxpool_forward(self, x, kernel, stride):
        """``i2v_i3d_maxpool_forward``: the variant's SAME-padded ceil-mode max pool (kT, k, k) / (sT, s, s) on x [B, T, H, W, C]."""
        self._require_cl(x, "i3d maxpool")
        B, T, H, W, C = x.shape
        od = self.maxpool_shape(kernel, stride, T, H, W)
        out = torch.empty(B, *od, C, dtype=torch.float32, device=x.device)
        _call("i2v_i3d_maxpool_forward", self._h, x.data_ptr(), B, T, H, W, C, kernel[0], kernel[1], stride[0], stride[1], out.data_ptr(),
                                         out.numel(), _stream())
        return out

    @_on_device
    def head_forward(self, x):
        """``i2v_i3d_head_forward``: x [B, T, 7, 7, 1024] -> (pooled [B, T', 1024], feats [B, 1024, T'], logits [B, num_classes])."""
        self._require_cl(x, "i3d head")
        B, T = x.shape[:2]
        nbytes = lib().i2v_i3d_head_workspace_bytes(self._h, B, T)
        if tuple(x.shape[2:]) != (7, 7, 1024) or nbytes == 0:
            raise I2VError(f"i3d head: expected [B,T,7,7,1024] with at least the average pool's time steps, got {tuple(x.shape)}")
        tp = T - (4 if self.dt_length == 32 else 2) + 1
        ws = self._scratch(nbytes, x.device)
        pooled = torch.empty(B, tp, 1024, dtype=torch.float32, device=x.device)
        feats = torch.empty(B, 1024, tp, dtype=torch.float32, device=x.device)
        logits = torch.empty(B, self.num_classes, dtype=torch.float32, device=x.device)
        _call("i2v_i3d_head_forward", self._h, x.data_ptr(), B, T, pooled.data_ptr(), feats.data_ptr(), logits.data_ptr(), *ws, _stream())
        return pooled, feats, logits


def fvd_stats_update(feats, total, gram):
    """``total`` [D] and ``gram`` [D, D] (float64, device) += the rows of ``feats`` [n, D] fp32 (``i2v_fvd_stats_update``): one owner per
    output element, the rows in order, no atomics."""
    _require_gpu(feats)
    n, d = feats.shape
    for t, shape in ((total, (d,)), (gram, (d, d))):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != feats.device:
            raise I2VError(f"fvd_stats_update: expected a contiguous float64 device tensor of shape {shape}")
    with torch.cuda.device(feats.device):
        _call("i2v_fvd_stats_update", feats.data_ptr(), n, d, total.data_ptr(), gram.data_ptr(), _stream())


def diversity_update(embed, acc):
    """``acc`` [2] (float64, device) += (sum over instances and ordered pairs i != j of mean_d (e_i - e_j)^2, number of such terms) of
    ``embed`` [N, R, D] fp32 (``i2v_diversity_update``): float64, one workgroup, fixed order."""
    _require_gpu(embed)
    if embed.dim() != 3 or embed.dtype != torch.float32 or not embed.is_contiguous():
        raise I2VError(f"diversity_update: expected contiguous fp32 embeddings [N,R,D], got {tuple(embed.shape)} {embed.dtype}")
    if not acc.is_cuda or acc.dtype != torch.float64 or not acc.is_contiguous() or tuple(acc.shape) != (2,) or acc.device != embed.device:
        raise I2VError("diversity_update: expected a contiguous float64 device tensor of shape (2,)")
    n, r, d = embed.shape
    with torch.cuda.device(embed.device):
        _call("i2v_diversity_update", embed.data_ptr(), n, r, d, acc.data_ptr(), _stream())


def i3d_input_stage(frames, denorm):
    """``i2v_i3d_input_stage``: frames [N, 3, H, W] on the device -> the stem input [N, 224, 224, 4] (channels-last, channel 3 zero)."""
    _require_gpu(frames)
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise I2VError(f"i3d_input_stage: expected frames [N,3,H,W], got {tuple(frames.shape)}")
    n, _, h, w = frames.shape
    out = torch.empty(n, 224, 224, 4, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _call("i2v_i3d_input_stage", frames.data_ptr(), n, h, w, int(bool(denorm)), out.data_ptr(), _stream())
    return out


VGG_TAPS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
VGG_TAP_CHANNELS = (64, 128, 256, 512, 512)
VGG_INPUT_LPIPS, VGG_INPUT_DIVERSITY = 0, 1


def _require_cl4(x, what):
    _require_gpu(x)
    if x.dim() != 4:
        raise I2VError(f"{what}: expected a contiguous fp32 channels-last tensor [N,H,W,C], got {tuple(x.shape)}")


def _reduce_ws(n, device):
    return torch.empty(lib().i2v_vgg_reduce_workspace_bytes(n), dtype=torch.uint8, device=device)


def _require_f64(t, shape, device, what):
    if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != device:
        raise I2VError(f"{what}: expected a contiguous float64 device tensor of shape {shape}")


class VGGSaved:
    """What ``NativeVGG.backward`` needs of one forward pass: the five taps and the buffer of the eight other post-ReLU activations."""

    def __init__(self, shape, taps, buf):
        self.shape, self.taps, self.buf = tuple(shape), list(taps), buf

    def activations(self):
        """The thirteen post-ReLU activations, channels-last [N, H', W', C], as views of the taps and of the buffer (where each lies:
        ``i2v_vgg_saved_layout``, the layer plan of csrc/i2v_vgg_plan.h)."""
        n = self.shape[0]
        lay = (VGGLayer * 13)()
        _call("i2v_vgg_saved_layout", n, self.shape[1], self.shape[2], lay)
        return [self.taps[L.tap] if L.tap >= 0 else
                self.buf[L.offset:L.offset + n * L.h * L.w * L.cout * 4].view(torch.float32).view(n, L.h, L.w, L.cout) for L in lay]


def _ptrs(tensors):
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class NativeVGG(_Handle):
    """Handle for ``i2v_vgg_*``: the VGG-16 ``features`` trunk of stage2_cINN/AE/modules/vgg16.py up to relu5_3, with the ``lin`` weights of
    LPIPS.py when the state_dict has them."""
    _PREFIX = "i2v_vgg"

    def __init__(self, device=None):
        self._create(device)
        self._bws = _Workspace()
        self.has_lin = False

    def load(self, state_dict):
        """torchvision keys ``features.N.{weight,bias}`` and, optionally, ``lin{0..4}.model.1.weight``; every other key is ignored."""
        self.has_lin = False
        super().load({k: v for k, v in state_dict.items()
                      if k.startswith("features.") or (k.startswith("lin") and k.endswith(".model.1.weight"))})
        self.has_lin = bool(lib().i2v_vgg_lin(self._h, 0))

    @staticmethod
    def tap_shapes(n, h, w):
        """Channels-last shapes [N, H', W', C] of the five taps for an [h, w] input."""
        return [(n, h >> k, w >> k, c) for k, c in enumerate(VGG_TAP_CHANNELS)]

    @_on_device
    def features(self, x, out=None, save=False, saved_buf=None):
        """``i2v_vgg_features``: x [N, H, W, 4] channels-last (``vgg_input_stage``) -> the five taps, channels-last [N, H', W', C].  ``out``:
        five caller-owned tensors of those shapes (the call only enqueues: it can be captured into a graph).  ``save=True``
        (``i2v_vgg_features_saved``): returns (taps, ``VGGSaved``) -- the same tap bits, and the state ``backward`` needs (``saved_buf``: a
        caller-owned uint8 buffer of ``saved_bytes`` for it)."""
        _require_cl4(x, "vgg features")
        n, h, w, c = x.shape
        nbytes = lib().i2v_vgg_workspace_bytes(self._h, n, h, w) if c == 4 else 0
        if nbytes == 0:
            raise I2VError(f"vgg features: expected [N,H,W,4] with H, W >= 16 (four pools), got {tuple(x.shape)}")
        ws = self._scratch(nbytes, x.device)
        shapes = self.tap_shapes(n, h, w)
        if out is None:
            out = [torch.empty(s, dtype=torch.float32, device=x.device) for s in shapes]
        for t, s in zip(out, shapes):
            _require_gpu(t)
            if tuple(t.shape) != s:
                raise I2VError(f"vgg features: expected a tap of shape {s}, got {tuple(t.shape)}")
        if save:
            nsaved = lib().i2v_vgg_saved_bytes(self._h, n, h, w)
            if saved_buf is None:
                saved_buf = torch.empty(nsaved, dtype=torch.uint8, device=x.device)
            if not saved_buf.is_cuda or saved_buf.dtype != torch.uint8 or not saved_buf.is_contiguous() or saved_buf.numel() < nsaved:
                raise I2VError(f"vgg features: the saved-state buffer must be a contiguous uint8 device tensor of at least {nsaved} bytes")
            _call("i2v_vgg_features_saved", self._h, x.data_ptr(), n, h, w, *[t.data_ptr() for t in out], saved_buf.data_ptr(), saved_buf.numel(),
                                            *ws, _stream())
            return list(out), VGGSaved(x.shape, out, saved_buf)
        _call("i2v_vgg_features", self._h, x.data_ptr(), n, h, w, *[t.data_ptr() for t in out], *ws, _stream())
        return list(out)

    def saved_bytes(self, n, h, w):
        return lib().i2v_vgg_saved_bytes(self._h, n, h, w)

    @_on_device
    def backward(self, tap_grads, saved, frames=False, out=None):
        """``i2v_vgg_backward``: five tap gradients (channels-last, the taps' shapes) and the ``VGGSaved`` of ``features(x, save=True)`` -> the
        gradient at x [N, H, W, 4], or with ``frames`` at the frames [N, 3, H, W] behind the LPIPS input stage.  Only enqueues (after the
        handle's first backward call, which packs the backward weights)."""
        if not isinstance(saved, VGGSaved):
            raise I2VError("vgg backward: no saved state -- run features(x, save=True); features(x) keeps only the taps")
        n, h, w, _ = saved.shape
        tap_grads = list(tap_grads)
        if len(tap_grads) != 5:
            raise I2VError(f"vgg backward: expected five tap gradients, got {len(tap_grads)}")
        for g, t in zip(tap_grads, saved.taps):
            _require_gpu(g)
            if g.shape != t.shape:
                raise I2VError(f"vgg backward: a tap gradient of shape {tuple(g.shape)} for a tap of shape {tuple(t.shape)}")
        shape = (n, 3, h, w) if frames else (n, h, w, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=saved.buf.device)
        _require_gpu(out)
        if tuple(out.shape) != shape:
            raise I2VError(f"vgg backward: expected an output of shape {shape}, got {tuple(out.shape)}")
        ws = self._scratch(lib().i2v_vgg_backward_workspace_bytes(self._h, n, h, w), out.device, self._bws)
        _call("i2v_vgg_backward", self._h, _ptrs(saved.taps), _ptrs(tap_grads), saved.buf.data_ptr(), saved.buf.numel(), n, h, w, out.data_ptr(),
                                  int(bool(frames)), *ws, _stream())
        return out

    @_on_device
    def lpips_backward(self, taps0, taps1, upstream, need0=True, need1=True, out0=None, out1=None):
        """``i2v_lpips_layer_backward`` over the five layers: ``upstream`` [N] float64 (the weight of every image's LPIPS value) -> (tap
        gradients of side 0, of side 1), each a list of five channels-last tensors or None when not needed."""
        if not self.has_lin:
            raise I2VError("lpips: the handle was loaded without lin{0..4}.model.1.weight")
        if not (need0 or need1):
            raise I2VError("lpips backward: no gradient requested")
        g = [lpips_layer_backward(a, b, lib().i2v_vgg_lin(self._h, k), upstream, need0, need1, None if out0 is None else out0[k],
                                  None if out1 is None else out1[k]) for k, (a, b) in enumerate(zip(taps0, taps1))]
        return [g0 for g0, _ in g] if need0 else None, [g1 for _, g1 in g] if need1 else None

    @_on_device
    def lpips(self, taps0, taps1):
        """Sum over the five layers of ``i2v_lpips_layer`` with the loaded ``lin`` weights: taps of two image batches -> float64 [N]."""
        if not self.has_lin:
            raise I2VError("lpips: the handle was loaded without lin{0..4}.model.1.weight")
        n = taps0[0].shape[0]
        out = torch.zeros(n, dtype=torch.float64, device=taps0[0].device)
        ws = _reduce_ws(n, out.device)
        for k, (a, b) in enumerate(zip(taps0, taps1)):
            lpips_layer(a, b, lib().i2v_vgg_lin(self._h, k), out, ws)
        return out


def vgg_input_stage(frames, mode, size=None, align_corners=False):
    """``i2v_vgg_input_stage``: frames [N, 3, H, W] in [-1, 1] on the device -> channels-last [N, Ho, Wo, 4] (channel 3 zero).  ``mode``
    VGG_INPUT_LPIPS: ScalingLayer, no resize; VGG_INPUT_DIVERSITY: ImageNet normalisation, then bilinear to ``size``."""
    _require_gpu(frames)
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise I2VError(f"vgg_input_stage: expected frames [N,3,H,W], got {tuple(frames.shape)}")
    n, _, h, w = frames.shape
    ho, wo = (h, w) if size is None else size
    out = torch.empty(n, ho, wo, 4, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _call("i2v_vgg_input_stage", frames.data_ptr(), n, h, w, mode, ho, wo, int(bool(align_corners)), out.data_ptr(), _stream())
    return out


def _host_f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


def vgg_conv_unit(x, weight, bias):
    """``i2v_vgg_conv_unit``: x [N, H, W, cin] channels-last on the device (cin = 3: [N, H, W, 4]), host ``weight`` [cout, cin, 3, 3] and
    ``bias`` [cout] -> relu(conv + bias) [N, H, W, cout]."""
    _require_cl4(x, "vgg_conv_unit")
    w, b = _host_f32(weight), _host_f32(bias)
    if w.ndim != 4 or w.shape[2:] != (3, 3) or b.shape != (w.shape[0],):
        raise I2VError(f"vgg_conv_unit: expected weight [cout,cin,3,3] and bias [cout], got {w.shape} / {b.shape}")
    cout, cin = w.shape[:2]
    n, h, wd, cs = x.shape
    if cs != (4 if cin == 3 else cin):
        raise I2VError(f"vgg_conv_unit: {cin} input channels need a tensor of {4 if cin == 3 else cin} stored channels, got {cs}")
    out = torch.empty(n, h, wd, cout, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call("i2v_vgg_conv_unit", x.data_ptr(), w.ctypes.data_as(c_void_p), b.ctypes.data_as(c_void_p), n, h, wd, cin, cout, out.data_ptr(),
                                   _stream())
    return out


def vgg_maxpool2(x):
    """``i2v_vgg_maxpool2``: MaxPool2d(2, 2) in floor mode on x [N, H, W, C] channels-last."""
    _require_cl4(x, "vgg_maxpool2")
    n, h, w, c = x.shape
    out = torch.empty(n, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call("i2v_vgg_maxpool2", x.data_ptr(), n, h, w, c, out.data_ptr(), _stream())
    return out


def vgg_dgrad_unit(g, weight, add=None, ymask=None, frames=False):
    """``i2v_vgg_dgrad_unit``: the input gradient of one 3x3 convolution of the trunk's kind.  g [N, H, W, cout] channels-last on the device,
    host ``weight`` [cout, cin, 3, 3] -> (dgrad + add) * (ymask > 0) [N, H, W, cin].  cin = 3 is the first-layer form: [N, H, W, 4], or with
    ``frames`` [N, 3, H, W] divided by ScalingLayer's scale."""
    _require_cl4(g, "vgg_dgrad_unit")
    w = _host_f32(weight)
    if w.ndim != 4 or w.shape[2:] != (3, 3):
        raise I2VError(f"vgg_dgrad_unit: expected weight [cout,cin,3,3], got {w.shape}")
    cout, cin = w.shape[:2]
    n, h, wd, cs = g.shape
    if cs != cout:
        raise I2VError(f"vgg_dgrad_unit: a gradient of {cs} channels for a weight of {cout} output channels")
    shape = (n, 3, h, wd) if frames else (n, h, wd, 4 if cin == 3 else cin)
    for t in (add, ymask):
        if t is not None:
            _require_cl4(t, "vgg_dgrad_unit")
            if tuple(t.shape) != shape:
                raise I2VError(f"vgg_dgrad_unit: expected an addend / mask of shape {shape}, got {tuple(t.shape)}")
    out = torch.empty(shape, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        _call("i2v_vgg_dgrad_unit", g.data_ptr(), w.ctypes.data_as(c_void_p), None if add is None else add.data_ptr(),
                                    None if ymask is None else ymask.data_ptr(), n, h, wd, cin, cout, out.data_ptr(), int(bool(frames)),
                                    _stream())
    return out


def vgg_maxpool2_backward(grad, y, add=None, relu_mask=False):
    """``i2v_vgg_maxpool2_backward``: grad [N, H/2, W/2, C], y [N, H, W, C] (the pool's input) -> [N, H, W, C]: the gradient at the first
    maximum of every window, zero elsewhere; then + ``add`` and, with ``relu_mask``, * (y > 0)."""
    _require_cl4(grad, "vgg_maxpool2_backward")
    _require_cl4(y, "vgg_maxpool2_backward")
    n, h, w, c = y.shape
    if tuple(grad.shape) != (n, h // 2, w // 2, c) or (add is not None and add.shape != y.shape):
        raise I2VError(f"vgg_maxpool2_backward: shapes {tuple(grad.shape)} / {tuple(y.shape)}")
    if add is not None:
        _require_cl4(add, "vgg_maxpool2_backward")
    out = torch.empty_like(y)
    with torch.cuda.device(y.device):
        _call("i2v_vgg_maxpool2_backward", grad.data_ptr(), y.data_ptr(), None if add is None else add.data_ptr(), int(bool(relu_mask)), n, h, w, c,
                                           out.data_ptr(), _stream())
    return out


def _lpips_layer_args(f0, f1, lin, what):
    """What the two one-layer calls check alike: f0, f1 channels-last taps of one shape; ``lin`` [C] a device tensor, or the device
    pointer ``i2v_vgg_lin`` gave (nothing to check).  -> (N, H * W, C, the pointer of lin)."""
    _require_cl4(f0, what)
    _require_cl4(f1, what)
    n, h, w, c = f0.shape
    lin_shape = tuple(lin.shape) if isinstance(lin, torch.Tensor) else (c,)
    if isinstance(lin, torch.Tensor):
        _require_gpu(lin)
        lin = lin.data_ptr()
    if f1.shape != f0.shape or lin_shape != (c,):
        raise I2VError(f"{what}: shapes {tuple(f0.shape)} / {tuple(f1.shape)} / {lin_shape}")
    return n, h * w, c, lin


def lpips_layer_backward(f0, f1, lin, upstream, need0=True, need1=True, out0=None, out1=None):
    """``i2v_lpips_layer_backward`` for one layer: f0, f1 [N, H, W, C] channels-last taps, lin [C] (or its pointer from ``i2v_vgg_lin``),
    upstream [N] float64 -> (g0, g1), None where not needed.  ``out0`` / ``out1``: caller-owned buffers of the taps' shape."""
    n, p, c, lin = _lpips_layer_args(f0, f1, lin, "lpips_layer_backward")
    _require_f64(upstream, (n,), f0.device, "lpips_layer_backward")
    g = [(torch.empty_like(f0) if out is None else out) if need else None for need, out in ((need0, out0), (need1, out1))]
    for t in g:
        if t is not None:
            _require_gpu(t)
            if t.shape != f0.shape:
                raise I2VError(f"lpips_layer_backward: a gradient buffer of shape {tuple(t.shape)} for a tap of shape {tuple(f0.shape)}")
    with torch.cuda.device(f0.device):
        _call("i2v_lpips_layer_backward", f0.data_ptr(), f1.data_ptr(), lin, upstream.data_ptr(), n, p, c,
                                          *[None if t is None else t.data_ptr() for t in g], _stream())
    return tuple(g)


def lpips_layer(f0, f1, lin, out, ws=None):
    """``out`` [N] (float64, device) += the LPIPS term of one layer (``i2v_lpips_layer``): f0, f1 [N, H, W, C] channels-last taps, lin [C]
    (or its pointer from ``i2v_vgg_lin``).  ``ws``: the reduction scratch of ``_reduce_ws(N)`` when the caller holds one."""
    n, p, c, lin = _lpips_layer_args(f0, f1, lin, "lpips_layer")
    _require_f64(out, (n,), f0.device, "lpips_layer")
    if ws is None:
        ws = _reduce_ws(n, f0.device)
    with torch.cuda.device(f0.device):
        _call("i2v_lpips_layer", f0.data_ptr(), f1.data_ptr(), lin, n, p, c, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())


def vgg_pairdiff_update(maps, acc):
    """``acc`` [2] (float64, device) += (sum over ordered pairs i != j of mean (f_i - f_j)^2, R (R - 1)) of ``maps`` [R, ...] fp32
    (``i2v_vgg_pairdiff_update``)."""
    _require_gpu(maps)
    if maps.dim() < 2:
        raise I2VError(f"vgg_pairdiff_update: expected maps [R, ...], got {tuple(maps.shape)}")
    _require_f64(acc, (2,), maps.device, "vgg_pairdiff_update")
    r = maps.shape[0]
    ws = _reduce_ws(1, maps.device)
    with torch.cuda.device(maps.device):
        _call("i2v_vgg_pairdiff_update", maps.data_ptr(), r, maps.numel() // r, acc.data_ptr(), ws.data_ptr(), ws.numel(), _stream())


INCEPTION_POOL_MAX_S2, INCEPTION_POOL_MAX_S1, INCEPTION_POOL_AVG = 0, 1, 2
INCEPTION_BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")
INCEPTION_MIN_SIDE = 75


class NativeInception(_Handle):
    """Handle for ``i2v_inception_*``: the FID Inception-v3 trunk of metrics/FID/inception.py (``fid_inception_v3`` cut into the four output
    blocks of ``InceptionV3``)."""
    _PREFIX = "i2v_inception"

    def __init__(self, device=None):
        self._create(device)

    def load(self, state_dict):
        """torchvision keys ``<unit>.conv.weight`` / ``<unit>.bn.{weight,bias,running_mean,running_var}``; ``num_batches_tracked``, ``fc.*`` and
        ``AuxLogits.*`` are ignored."""
        super().load({k: v for k, v in state_dict.items()
                      if not (k.endswith("num_batches_tracked") or k.startswith("fc.") or k.startswith("AuxLogits."))})

    def block_shape(self, n, h, w, block):
        """Channels-last shape of output block 0..3 for an [h, w] trunk input: [N, H', W', C], block 3 [N, 2048]."""
        dims = (c_int32 * 3)()
        _call("i2v_inception_block_shape", self._h, h, w, block, dims)
        return (n, dims[2]) if block == 3 else (n, dims[0], dims[1], dims[2])

    @_on_device
    def features(self, x, blocks=(3,), out=None):
        """``i2v_inception_features``: x [N, H, W, 4] channels-last (``inception_input_stage``) -> the requested blocks, channels-last, in
        ascending order.  ``out``: caller-owned tensors of those shapes (the call only enqueues: it can be captured into a graph)."""
        _require_cl4(x, "inception features")
        n, h, w, c = x.shape
        blocks = sorted(set(int(b) for b in blocks))
        if not blocks or blocks[0] < 0 or blocks[-1] > 3:
            raise I2VError(f"inception features: output blocks must be a non-empty subset of 0..3, got {blocks}")
        if c != 4 or h < INCEPTION_MIN_SIDE or w < INCEPTION_MIN_SIDE:
            raise I2VError(f"inception features: expected [N,H,W,4] with H, W >= {INCEPTION_MIN_SIDE} (the minimum that leaves a 1 x 1 map in front of "
                           f"the final pool), got {tuple(x.shape)}")
        nbytes = lib().i2v_inception_workspace_bytes(self._h, n, h, w, blocks[-1])
        if nbytes == 0:
            raise I2VError(f"inception features: no buffer plan for {tuple(x.shape)}: {lib().i2v_last_error().decode(errors='replace')}")
        ws = self._scratch(nbytes, x.device)
        shapes = [self.block_shape(n, h, w, b) for b in blocks]
        if out is None:
            out = [torch.empty(s, dtype=torch.float32, device=x.device) for s in shapes]
        ptr = [None] * 4
        for b, t, s in zip(blocks, out, shapes):
            _require_gpu(t)
            if tuple(t.shape) != s:
                raise I2VError(f"inception features: expected block {b} of shape {s}, got {tuple(t.shape)}")
            ptr[b] = t.data_ptr()
        _call("i2v_inception_features", self._h, x.data_ptr(), n, h, w, *ptr, *ws, _stream())
        return list(out)

    def mixed_shape(self, block, h, w):
        """(cin, cout, (H', W')) of Mixed block ``block`` (index into INCEPTION_BLOCKS) on an [h, w] map."""
        cin, cout, hw = c_int32(), c_int32(), (c_int32 * 2)()
        _call("i2v_inception_mixed_shape", self._h, block, h, w, ctypes.byref(cin), ctypes.byref(cout), hw)
        return cin.value, cout.value, (hw[0], hw[1])

    @_on_device
    def mixed(self, block, x, out=None):
        """``i2v_inception_mixed_forward``: x [N, H, W, cin] channels-last -> [N, H', W', cout]; ``out``: a caller-owned tensor (every element of
        it is written)."""
        _require_cl4(x, "inception mixed")
        n, h, w, c = x.shape
        cin, cout, (ho, wo) = self.mixed_shape(block, h, w)
        if c != cin:
            raise I2VError(f"inception mixed: {INCEPTION_BLOCKS[block]} takes {cin} channels, got {c}")
        if out is None:
            out = torch.empty(n, ho, wo, cout, dtype=torch.float32, device=x.device)
        _require_gpu(out)
        if tuple(out.shape) != (n, ho, wo, cout):
            raise I2VError(f"inception mixed: expected an output of shape {(n, ho, wo, cout)}, got {tuple(out.shape)}")
        ws = torch.empty(max(lib().i2v_inception_mixed_workspace_bytes(self._h, block, n, h, w), 256), dtype=torch.uint8, device=x.device)
        _call("i2v_inception_mixed_forward", self._h, block, x.data_ptr(), n, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return out


def inception_input_stage(frames, resize=True, normalize=False):
    """``i2v_inception_input_stage``: frames [N, 3, H, W] on the device -> channels-last [N, 299, 299, 4] (bilinear, align_corners=False) or, without
    ``resize``, [N, H, W, 4]; ``normalize``: 2 x - 1 behind the resize.  Channel 3 is zero."""
    _require_gpu(frames)
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise I2VError(f"inception_input_stage: expected frames [N,3,H,W], got {tuple(frames.shape)}")
    n, _, h, w = frames.shape
    ho, wo = (299, 299) if resize else (h, w)
    out = torch.empty(n, ho, wo, 4, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _call("i2v_inception_input_stage", frames.data_ptr(), n, h, w, int(bool(resize)), int(bool(normalize)), out.data_ptr(), _stream())
    return out


def inception_conv_unit(x, weight, bn, stride=1, padding=(0, 0), in_off=0, out=None, out_off=0):
    """``i2v_inception_conv_unit``: one BasicConv2d.  x [N, H, W, CS] channels-last on the device, of which channels [in_off, in_off + cin) are
    read (cin = 3: four stored channels); host ``weight`` [cout, cin, kh, kw] and ``bn`` = (weight, bias, running_mean, running_var), each
    [cout]; eps 0.001.  Writes channels [out_off, out_off + cout) of ``out`` [N, H', W', OCS] (default: a new tensor of cout channels)."""
    _require_cl4(x, "inception_conv_unit")
    w = _host_f32(weight)
    vec = [_host_f32(v) for v in bn]
    if w.ndim != 4 or len(vec) != 4 or any(v.shape != (w.shape[0],) for v in vec):
        raise I2VError(f"inception_conv_unit: expected weight [cout,cin,kh,kw] and four BatchNorm vectors [cout], got {w.shape} / {[v.shape for v in vec]}")
    cout, cin, kh, kw = w.shape
    n, h, wd, cs = x.shape
    ph, pw = padding
    ho, wo = (h + 2 * ph - kh) // stride + 1, (wd + 2 * pw - kw) // stride + 1
    if out is None:
        out = torch.empty(n, max(ho, 0), max(wo, 0), cout, dtype=torch.float32, device=x.device)
    _require_cl4(out, "inception_conv_unit")
    if tuple(out.shape[:3]) != (n, max(ho, 0), max(wo, 0)):
        raise I2VError(f"inception_conv_unit: expected an output [N,{ho},{wo},C], got {tuple(out.shape)}")
    with torch.cuda.device(x.device):
        _call("i2v_inception_conv_unit", x.data_ptr(), n, h, wd, cs, in_off, w.ctypes.data_as(c_void_p), *[v.ctypes.data_as(c_void_p) for v in vec],
                                         cin, cout, kh, kw, stride, ph, pw, out.data_ptr(), out.shape[3], out_off, out.numel(), _stream())
    return out


def inception_pool(x, kind, out=None, out_off=0):
    """``i2v_inception_pool``: one 3 x 3 pool of ``kind`` (INCEPTION_POOL_*) on x [N, H, W, C] channels-last; writes channels
    [out_off, out_off + C) of ``out`` (default: a new tensor of C channels)."""
    _require_cl4(x, "inception_pool")
    n, h, w, c = x.shape
    s, p = (2, 0) if kind == INCEPTION_POOL_MAX_S2 else (1, 1)
    ho, wo = (h + 2 * p - 3) // s + 1, (w + 2 * p - 3) // s + 1
    if out is None:
        out = torch.empty(n, max(ho, 0), max(wo, 0), c, dtype=torch.float32, device=x.device)
    _require_cl4(out, "inception_pool")
    if tuple(out.shape[:3]) != (n, max(ho, 0), max(wo, 0)):
        raise I2VError(f"inception_pool: expected an output [N,{ho},{wo},C], got {tuple(out.shape)}")
    with torch.cuda.device(x.device):
        _call("i2v_inception_pool", x.data_ptr(), n, h, w, c, kind, out.data_ptr(), out.shape[3], out_off, out.numel(), _stream())
    return out


def inception_global_avg(x):
    """``i2v_inception_global_avg``: AdaptiveAvgPool2d((1, 1)) on x [N, H, W, C] channels-last -> [N, C]."""
    _require_cl4(x, "inception_global_avg")
    n, h, w, c = x.shape
    out = torch.empty(n, c, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call("i2v_inception_global_avg", x.data_ptr(), n, h, w, c, out.data_ptr(), _stream())
    return out


def _recon_view(x, what):
    """(tensor, B, T, C, H, W, batch stride in floats) of a float32 device tensor [B, T, C, H, W] or [N, C, H, W] whose [T, C, H, W] blocks are
    contiguous (any batch stride: the view ``seq[:, 1:]`` is taken in place); anything else on the device is made contiguous."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise I2VError(f"{what}: expected frames [B,T,C,H,W] or [N,C,H,W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if not x.is_cuda:
        raise I2VError(f"{what}: libi2v_hip kernels need tensors on a HIP device (got a CPU tensor); this package has no CPU fallback")
    if x.dtype != torch.float32:
        raise I2VError(f"{what}: expected float32 frames, got {x.dtype}")
    if x.dim() == 4:
        x = x.unsqueeze(1)
    view = NativeDecoder._sample_strided(x, x.shape[1:])
    if view is None:
        x = x.contiguous()
        view = (x.data_ptr(), x[0].numel())
    return (x, *x.shape, view[1])


def _recon_args(pred, target, what):
    p, t = _recon_view(pred, what), _recon_view(target, what)
    if p[1:6] != t[1:6] or p[0].device != t[0].device:
        raise I2VError(f"{what}: pred {tuple(pred.shape)} on {pred.device} and target {tuple(target.shape)} on {target.device} do not match")
    shape = tuple(int(v) for v in p[1:6])
    nbytes = int(lib().i2v_recon_workspace_bytes(*shape))
    if nbytes == 0:
        raise I2VError(f"{what}: frames of shape {shape} are refused (empty, or too large)")
    return p[0], t[0], shape, int(p[6]), int(t[6]), torch.empty(nbytes, dtype=torch.uint8, device=p[0].device)


def recon_range(pred, target):
    """``i2v_recon_range``: float64 [4] on the device = min(pred), max(pred), min(target), max(target)."""
    p, t, shape, pbs, tbs, ws = _recon_args(pred, target, "recon_range")
    out = torch.empty(4, dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        _call("i2v_recon_range", p.data_ptr(), t.data_ptr(), *shape, pbs, tbs, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


def recon_stats(pred, target, data_range=None):
    """``i2v_recon_stats`` (behind ``i2v_recon_range`` when ``data_range`` is None) on two frame tensors [B, T, C, H, W] (or [N, C, H, W]) ->
    (scalars float64 [5]: L1 mean, MSE, PSNR, SSIM, number of SSIM terms; per_image float64 [N, 3]: sum |p - t|, sum (p - t)^2, sum of the
    SSIM map; range float64 [4] or None).  Everything stays on the device and nothing synchronises."""
    fixed = 0.0
    if data_range is not None:
        fixed = float(data_range)
        if not fixed > 0.0:
            raise I2VError(f"recon_stats: data_range must be a positive number or None, got {data_range!r}")
    p, t, shape, pbs, tbs, ws = _recon_args(pred, target, "recon_stats")
    n = shape[0] * shape[1]
    scalars = torch.empty(5, dtype=torch.float64, device=p.device)
    per_image = torch.empty(n, 3, dtype=torch.float64, device=p.device)
    rng = None
    with torch.cuda.device(p.device):
        if data_range is None:
            rng = torch.empty(4, dtype=torch.float64, device=p.device)
            _call("i2v_recon_range", p.data_ptr(), t.data_ptr(), *shape, pbs, tbs, rng.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        _call("i2v_recon_stats", p.data_ptr(), t.data_ptr(), *shape, pbs, tbs, None if rng is None else rng.data_ptr(), fixed,
                                 per_image.data_ptr(), scalars.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return scalars, per_image, rng


def kl_normal(mu, logvar):
    """``i2v_kl_normal``: -0.5 * mean_b sum_d (1 + logvar - mu^2 - exp(logvar)) of mu, logvar [B, D] fp32 -> float64 0-d on the device."""
    _require_gpu(mu, logvar)
    if mu.dim() != 2 or mu.shape != logvar.shape or mu.device != logvar.device:
        raise I2VError(f"kl_normal: expected mu and logvar [B,D] on one device, got {tuple(mu.shape)} / {tuple(logvar.shape)}")
    out = torch.empty(1, dtype=torch.float64, device=mu.device)
    with torch.cuda.device(mu.device):
        _call("i2v_kl_normal", mu.data_ptr(), logvar.data_ptr(), mu.shape[0], mu.shape[1], out.data_ptr(), _stream())
    return out[0]


# ---------------------------------------------------------------------------------------------------- patch discriminator (stage 1)
PATCHDISC_ITERATE, PATCHDISC_INIT_ACTNORM, PATCHDISC_SAVE = 1, 2, 4
HINGE_DISC, HINGE_GEN = 0, 1


def _opt(t):
    return None if t is None else t.data_ptr()


class _BoundHandle(_Handle):
    """A handle that packs nothing on the host: ``bind`` hands over the DEVICE pointers of the module's parameters and buffers (read in
    place) and ``bind_grads`` those of their gradient tensors.  The two are bound apart: a fresh gradient buffer per backward re-binds
    the gradients alone.  ``bound_ptrs`` / ``bound_grad_ptrs`` are the pointers last handed over; ``_keep`` / ``_keep_grads`` keep their
    tensors alive."""
    bound_ptrs = bound_grad_ptrs = _keep = _keep_grads = None

    def load(self, state_dict):
        raise I2VError(f"{type(self).__name__} packs nothing: bind() hands over the module's own parameters")

    @staticmethod
    def _items(tensors):
        keep = [k.encode() for k in tensors]
        for t in tensors.values():
            _require_gpu(t)
        return (_Tensor * len(keep))(*[_Tensor(kb, t.data_ptr(), t.numel(), I2V_F32) for kb, t in zip(keep, tensors.values())]), keep

    def bind(self, tensors):
        """tensors: {state_dict key: float32 device tensor} of the parameters and the spectral-norm buffers."""
        with self._on(*tensors.values()):
            arr, keep = self._items(tensors)
            _call(f"{self._PREFIX}_bind", self._h, arr, len(keep))
        self.bound_ptrs = tuple(t.data_ptr() for t in tensors.values())
        self._keep = tensors

    def bind_grads(self, grads):
        """grads: {key: gradient tensor} of the trained parameters, or None."""
        if grads is None:
            _call(f"{self._PREFIX}_bind_grads", self._h, None, 0)
        else:
            with self._on(*grads.values()):
                arr, keep = self._items(grads)
                _call(f"{self._PREFIX}_bind_grads", self._h, arr, len(keep))
        self.bound_grad_ptrs = None if grads is None else tuple(g.data_ptr() for g in grads.values())
        self._keep_grads = grads


class _Res3DHandle(_BoundHandle):
    """What the two handles on the 3-D ResNet training trunk (csrc/i2v_res3d_net.h) share: the clip check and the views of ``saved``."""
    _NAME = None                  # the network, for messages
    _INT32_KINDS = frozenset()    # the kinds of ``saved_maps`` that hold int32

    def _shape(self, x):
        if x.dim() != 5 or x.shape[1] != 3:
            raise I2VError(f"{self._NAME}: expected clips [N, 3, T, H, W], got {tuple(x.shape)}")
        n, _, t, h, w = x.shape
        return n, t, h, w

    def saved_bytes(self, n, t, h, w):
        return int(getattr(lib(), self._PREFIX + "_saved_bytes")(self._h, n, t, h, w))

    def workspace_bytes(self, n, t, h, w):
        return int(getattr(lib(), self._PREFIX + "_workspace_bytes")(self._h, n, t, h, w))

    def saved_maps(self, saved, shape):
        """{(kind, conv): view of ``saved`` [N, T, H, W, C]} (the network's kinds; the pool's maps have conv -1), for the tests."""
        n, _, t, h, w = shape
        cnt, kind, conv, dims, off = c_int32(), (c_int32 * 64)(), (c_int32 * 64)(), (c_int32 * 256)(), (c_int64 * 64)()
        _call(self._PREFIX + "_saved_layout", self._h, n, t, h, w, ctypes.byref(cnt), kind, conv, dims, off)
        out = {}
        for e in range(cnt.value):
            shp = (n, *dims[4 * e: 4 * e + 4])
            flat = saved.view(torch.int32 if kind[e] in self._INT32_KINDS else torch.float32)
            out[(kind[e], conv[e])] = flat[off[e] // 4: off[e] // 4 + int(np.prod(shp))].view(shp)
        return out


def flat_param_grads(module, device):
    """{parameter name: gradient tensor} for every parameter of ``module``: views of one flat fp32 allocation on ``device``, each
    starting on a multiple of 4 floats."""
    sizes = [(p.numel() + 3) // 4 * 4 for p in module.parameters()]
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=device)
    return {k: v[:p.numel()].view(p.shape) for (k, p), v in zip(module.named_parameters(), flat.split(sizes))}


def bind_in_place(handle, tensors, grads=None):
    """Binds a _BoundHandle to the storage of ``tensors`` as it is now and, when ``grads`` ({parameter name: tensor}) is given, to those
    gradient tensors, each only if its pointers moved; the two bindings are kept apart, so a forward never re-binds because of a
    backward's gradient buffer."""
    if handle.bound_ptrs != tuple(t.data_ptr() for t in tensors.values()):
        handle.bind({k: t.detach().view(-1) for k, t in tensors.items()})
    if grads is not None and handle.bound_grad_ptrs != tuple(g.data_ptr() for g in grads.values()):
        handle.bind_grads({k: g.detach().view(-1) for k, g in grads.items()})
    return handle


class NativePatchDisc(_BoundHandle):
    """Handle for ``i2v_patchdisc_*`` (include/i2v_hip_disc.h): NLayerDiscriminator forward and backward.  It packs nothing on the
    host: ``bind`` hands over the DEVICE pointers of the module's parameters and buffers (read in place; ``weight_u``, ``weight_v``,
    ``loc`` and ``scale`` are updated in place) and of their gradient tensors."""
    _PREFIX = "i2v_patchdisc"

    def __init__(self, in_channels=3, ndf=64, n_layers=3, use_actnorm=True, spectral_norm=True, device=None):
        cfg = PatchDiscCfg(int(in_channels), int(ndf), int(n_layers), int(bool(use_actnorm)), int(bool(spectral_norm)))
        self._create(device, ctypes.byref(cfg))

    def out_shape(self, h, w):
        ho, wo = c_int32(), c_int32()
        _call("i2v_patchdisc_out_shape", self._h, int(h), int(w), ctypes.byref(ho), ctypes.byref(wo))
        return ho.value, wo.value

    def _shape(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise I2VError(f"patch discriminator: expected frames [N, 3, H, W], got {tuple(x.shape)}")
        n, _, h, w = x.shape
        return n, h, w, self.out_shape(h, w)

    def saved_bytes(self, n, h, w):
        return int(lib().i2v_patchdisc_saved_bytes(self._h, n, h, w))

    def saved_activations(self, saved, shape):
        """[(activation, pre-ActNorm output or None) per conv but the last], views of ``saved`` [N, Ho, Wo, Cout], for the tests."""
        n, _, h, w = shape
        nc, ho, wo, co = c_int32(), (c_int32 * 8)(), (c_int32 * 8)(), (c_int32 * 8)()
        ao, po = (c_int64 * 8)(), (c_int64 * 8)()
        _call("i2v_patchdisc_saved_layout", self._h, n, h, w, ctypes.byref(nc), ho, wo, co, ao, po)
        flat = saved.view(torch.float32)
        view = lambda off, i: None if off < 0 else flat[off // 4: off // 4 + n * ho[i] * wo[i] * co[i]].view(n, ho[i], wo[i], co[i])
        return [(view(ao[i], i), view(po[i], i)) for i in range(nc.value - 1)]

    @_on_device
    def forward(self, x, iterate=False, init_actnorm=False, save=False):
        """-> pred [N, 1, Ho, Wo], or (pred, saved) with ``save``: the uint8 buffer that belongs to this pass and goes to ``backward``."""
        _require_gpu(x)
        n, h, w, (ho, wo) = self._shape(x)
        ws = self._scratch(lib().i2v_patchdisc_workspace_bytes(self._h, n, h, w), x.device)
        saved = torch.empty(self.saved_bytes(n, h, w), dtype=torch.uint8, device=x.device) if save else None
        pred = torch.empty(n, 1, ho, wo, dtype=torch.float32, device=x.device)
        flags = (PATCHDISC_ITERATE if iterate else 0) | (PATCHDISC_INIT_ACTNORM if init_actnorm else 0) | (PATCHDISC_SAVE if save else 0)
        _call("i2v_patchdisc_forward", self._h, x.data_ptr(), n, h, w, flags, pred.data_ptr(), _opt(saved), 0 if saved is None else saved.numel(), *ws,
              _stream())
        return (pred, saved) if save else pred

    @_on_device
    def backward(self, d_pred, saved, shape, need_dx=True, param_grads=True, accumulate=False):
        """``shape``: the (N, 3, H, W) of the forward's input.  -> d_x [N, 3, H, W] or None; the parameter gradients go to the bound
        gradient tensors, written or (``accumulate``) added."""
        _require_gpu(d_pred)
        n, _, h, w = shape
        ws = self._scratch(lib().i2v_patchdisc_workspace_bytes(self._h, n, h, w), d_pred.device)
        dx = torch.empty(n, 3, h, w, dtype=torch.float32, device=d_pred.device) if need_dx else None
        _call("i2v_patchdisc_backward", self._h, d_pred.data_ptr(), saved.data_ptr(), saved.numel(), n, h, w, _opt(dx), int(bool(param_grads)),
              int(bool(accumulate)), *ws, _stream())
        return dx


def patchdisc_hinge(fake, real=None, mode="disc", need_grads=True):
    """``hinge_loss`` with its gradient -> (out, d_fake, d_real): out float64 [3] = (loss, mean(real), mean(fake)) on the device."""
    _require_gpu(fake, real)
    if (mode == "disc") != (real is not None) or (real is not None and real.shape != fake.shape):
        raise I2VError("patchdisc_hinge: 'disc' takes fake and real of one shape, 'gen' fake alone")
    with torch.cuda.device(fake.device):
        out = torch.zeros(3, dtype=torch.float64, device=fake.device)
        d_fake = torch.empty_like(fake) if need_grads else None
        d_real = torch.empty_like(real) if need_grads and real is not None else None
        _call("i2v_patchdisc_hinge", fake.data_ptr(), _opt(real), fake.numel(), HINGE_DISC if mode == "disc" else HINGE_GEN, out.data_ptr(),
              _opt(d_fake), _opt(d_real), _stream())
    return out, d_fake, d_real


def patchdisc_wgrad_plan(cout, cin, positions):
    """(slices, slice_len) of the weight gradient's position split: a pure host function of the shape."""
    s, l = c_int32(), c_int32()
    _call("i2v_patchdisc_wgrad_plan", int(cout), int(cin), int(positions), ctypes.byref(s), ctypes.byref(l))
    return s.value, l.value


def _pd_ws(n, hi, wi, cin, cout, device):
    return torch.empty(int(lib().i2v_patchdisc_unit_workspace_bytes(n, hi, wi, cin, cout)), dtype=torch.uint8, device=device)


def _pd_geom(x, weight, stride):
    n, hi, wi, cs = x.shape
    cout, cin = weight.shape[:2]
    if cs != (4 if cin == 3 else cin) or tuple(weight.shape[2:]) != (4, 4):
        raise I2VError(f"patch discriminator unit: map {tuple(x.shape)} against weight {tuple(weight.shape)}")
    return n, hi, wi, cin, cout, (hi - 2) // stride + 1, (wi - 2) // stride + 1


def patchdisc_conv_unit(x, weight, bias, loc=None, scale=None, stride=2, lrelu=False, want_pre=False):
    """x [N, H, W, C] channels-last (C = 4 for cin 3) -> out [N, Ho, Wo, Cout] (and the pre-ActNorm conv output with ``want_pre``)."""
    _require_gpu(x, weight, bias, loc, scale)
    n, hi, wi, cin, cout, ho, wo = _pd_geom(x, weight, stride)
    with torch.cuda.device(x.device):
        ws = _pd_ws(n, hi, wi, cin, cout, x.device)
        out = torch.empty(n, ho, wo, cout, dtype=torch.float32, device=x.device)
        pre = torch.empty_like(out) if want_pre else None
        _call("i2v_patchdisc_conv_unit", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), _opt(loc), _opt(scale), n, hi, wi, cin, cout, stride,
              int(bool(lrelu)), out.data_ptr(), _opt(pre), ws.data_ptr(), ws.numel(), _stream())
    return (out, pre) if want_pre else out


def patchdisc_dgrad_unit(g, weight, in_hw, act=None, scale=None, stride=2, frames=False):
    """g [N, Ho, Wo, Cout] -> the gradient at the conv's input [N, H, W, Cin] (cin 3: 4 channels, or [N, 3, H, W] with ``frames``)."""
    _require_gpu(g, weight, act, scale)
    n, (hi, wi), (cout, cin) = g.shape[0], in_hw, weight.shape[:2]
    with torch.cuda.device(g.device):
        ws = _pd_ws(n, hi, wi, cin, cout, g.device)
        out = torch.empty((n, 3, hi, wi) if frames else (n, hi, wi, 4 if cin == 3 else cin), dtype=torch.float32, device=g.device)
        _call("i2v_patchdisc_dgrad_unit", g.data_ptr(), weight.data_ptr(), _opt(act), _opt(scale), n, hi, wi, cin, cout, stride, out.data_ptr(),
              int(bool(frames)), ws.data_ptr(), ws.numel(), _stream())
    return out


def patchdisc_wgrad_unit(g, x, weight, act=None, scale=None, u=None, v=None, sigma=None, stride=2, dweight=None, dbias=None):
    """-> (dweight [Cout, Cin, 4, 4], dbias [Cout]); given ``dweight`` / ``dbias`` the result is ADDED to them."""
    _require_gpu(g, x, weight, act, scale, u, v, sigma, dweight, dbias)
    n, hi, wi, cin, cout, _, _ = _pd_geom(x, weight, stride)
    accumulate = dweight is not None
    with torch.cuda.device(g.device):
        ws = _pd_ws(n, hi, wi, cin, cout, g.device)
        if not accumulate:
            dweight, dbias = torch.empty_like(weight), torch.empty(cout, dtype=torch.float32, device=g.device)
        _call("i2v_patchdisc_wgrad_unit", g.data_ptr(), _opt(act), _opt(scale), x.data_ptr(), weight.data_ptr(), _opt(u), _opt(v), _opt(sigma), n, hi, wi,
              cin, cout, stride, int(accumulate), dweight.data_ptr(), dbias.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return dweight, dbias


def patchdisc_head_unit(x, weight, bias, g=None):
    """The cout = 1 conv: x [N, H, W, C] -> out [N, H-1, W-1]; with g also (dx, dweight, dbias)."""
    _require_gpu(x, weight, bias, g)
    n, hi, wi, cin = x.shape
    with torch.cuda.device(x.device):
        ws = _pd_ws(n, hi, wi, cin, 1, x.device)
        out = torch.empty(n, hi - 1, wi - 1, dtype=torch.float32, device=x.device)
        dx, dw, db = (torch.empty_like(x), torch.empty_like(weight), torch.empty(1, dtype=torch.float32, device=x.device)) if g is not None else (None,) * 3
        _call("i2v_patchdisc_head_unit", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), _opt(g), n, hi, wi, cin, out.data_ptr(), _opt(dx), _opt(dw),
              _opt(db), ws.data_ptr(), ws.numel(), _stream())
    return out if g is None else (out, dx, dw, db)


def patchdisc_power_iteration_unit(weight, u, v, iterate=True):
    """weight [rows, cols]; u, v updated in place when ``iterate``; -> sigma [1]."""
    _require_gpu(weight, u, v)
    rows, cols = weight.shape
    with torch.cuda.device(weight.device):
        ws = torch.empty(8 * (rows + cols) + 1024, dtype=torch.uint8, device=weight.device)
        sigma = torch.empty(1, dtype=torch.float32, device=weight.device)
        _call("i2v_patchdisc_power_iteration_unit", weight.data_ptr(), u.data_ptr(), v.data_ptr(), rows, cols, int(bool(iterate)), sigma.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream())
    return sigma


def patchdisc_actnorm_init_unit(pre):
    """pre [M, C] -> (loc [C], scale [C])."""
    _require_gpu(pre)
    m, c = pre.shape
    with torch.cuda.device(pre.device):
        loc, scale = torch.empty(c, dtype=torch.float32, device=pre.device), torch.empty(c, dtype=torch.float32, device=pre.device)
        _call("i2v_patchdisc_actnorm_init_unit", pre.data_ptr(), m, c, loc.data_ptr(), scale.data_ptr(), _stream())
    return loc, scale


# ---------------------------------------------------------------------------------------------------------------- temporal discriminator
DISC3D_ITERATE, DISC3D_SAVE = 1, 2
DISC3D_CONV_OUT, DISC3D_ACT, DISC3D_POOL_OUT, DISC3D_POOL_ARGMAX = 0, 1, 2, 3
FMAP_METRICS = {"L1": 0, "L2": 1}


def _ptr_array(tensors, count=4):
    """void*[count] of the tensors' device pointers (None -> NULL), or None when ``tensors`` is None."""
    if tensors is None:
        return None
    return (c_void_p * count)(*[None if t is None else t.data_ptr() for t in tensors])


class NativeDisc3D(_Res3DHandle):
    """Handle for ``i2v_disc3d_*`` (include/i2v_hip_disc3d.h): resnet3D.Discriminator forward and backward.  It packs nothing on the
    host: ``bind`` hands over the DEVICE pointers of the module's parameters and buffers (read in place; ``weight_u`` and ``weight_v``
    are updated in place) and ``bind_grads`` those of their gradient tensors.  Feature maps are channels-last [N, T, H, W, C]."""
    _PREFIX, _NAME, _INT32_KINDS = "i2v_disc3d", "temporal discriminator", frozenset({DISC3D_POOL_ARGMAX})

    def __init__(self, channels, stride_s, stride_t, use_max_pool=True, spectral_norm=True, res_type=18, device=None):
        if len(channels) != 5 or len(stride_s) != 4 or len(stride_t) != 4:
            raise I2VError(f"temporal discriminator: {len(channels)} widths with {len(stride_s)} / {len(stride_t)} strides (5 and 4 are built)")
        cfg = Disc3DCfg(int(res_type), (c_int32 * 5)(*map(int, channels)), (c_int32 * 4)(*map(int, stride_s)), (c_int32 * 4)(*map(int, stride_t)),
                        int(bool(use_max_pool)), int(bool(spectral_norm)))
        self._create(device, ctypes.byref(cfg))

    def out_shape(self, t, h, w):
        """[(t, h, w, c)] of the four feature maps; raises with the final map in the message unless the net ends on [1, 4, 4]."""
        s = (c_int32 * 16)()
        _call("i2v_disc3d_out_shape", self._h, int(t), int(h), int(w), s)
        return [tuple(s[4 * i: 4 * i + 4]) for i in range(4)]

    @_on_device
    def forward(self, x, iterate=False, save=False, want_fmaps=True):
        """x [N, 3, T, H, W] -> (pred [N, 1], fmaps or None, saved or None)."""
        _require_gpu(x)
        n, t, h, w = self._shape(x)
        shapes = self.out_shape(t, h, w)
        ws = self._scratch(self.workspace_bytes(n, t, h, w), x.device)
        saved = torch.empty(self.saved_bytes(n, t, h, w), dtype=torch.uint8, device=x.device) if save else None
        pred = torch.empty(n, 1, dtype=torch.float32, device=x.device)
        fmaps = [torch.empty(n, *s, dtype=torch.float32, device=x.device) for s in shapes] if want_fmaps else None
        flags = (DISC3D_ITERATE if iterate else 0) | (DISC3D_SAVE if save else 0)
        _call("i2v_disc3d_forward", self._h, x.data_ptr(), n, t, h, w, flags, pred.data_ptr(), _ptr_array(fmaps), _opt(saved),
              0 if saved is None else saved.numel(), *ws, _stream())
        return pred, fmaps, saved

    @_on_device
    def backward(self, d_pred, d_fmaps, saved, shape, need_dx=True, param_grads=True, accumulate=False):
        """``shape``: the (N, 3, T, H, W) of the forward's input; d_pred [N, 1] or None; d_fmaps: None or four channels-last tensors / None.
        -> d_x [N, 3, T, H, W] or None; the parameter gradients go to the bound gradient tensors, written or (``accumulate``) added."""
        _require_gpu(d_pred, *(d_fmaps or ()))
        n, _, t, h, w = shape
        ws = self._scratch(self.workspace_bytes(n, t, h, w), saved.device)
        dx = torch.empty(n, 3, t, h, w, dtype=torch.float32, device=saved.device) if need_dx else None
        _call("i2v_disc3d_backward", self._h, _opt(d_pred), _ptr_array(d_fmaps), saved.data_ptr(), saved.numel(), n, t, h, w, _opt(dx),
              int(bool(param_grads)), int(bool(accumulate)), *ws, _stream())
        return dx

    # ---- the gradient penalty with its gradient (include/i2v_hip_disc3d_gp.h)
    def gp_saved_bytes(self, n, t, h, w):
        return int(lib().i2v_disc3d_gp_saved_bytes(self._h, n, t, h, w))

    def gp_workspace_bytes(self, n, t, h, w):
        return int(lib().i2v_disc3d_gp_workspace_bytes(self._h, n, t, h, w))

    @_on_device
    def gp_backward(self, saved, shape, scale=1.0, scale_dev=None, accumulate=False, gp_saved=None, l_gp=None):
        """From the ``saved`` of a saved forward on clips of ``shape`` (N, 3, T, H, W): the penalty's value and ``scale`` (times the
        device float ``scale_dev`` [1] when given) times its gradient at every parameter, written or (``accumulate``) added to the bound
        gradient tensors.  -> (L_GP as a float64 0-d device tensor, gp_saved: the tangent's maps, see ``gp_saved_maps``).  ``gp_saved`` /
        ``l_gp``: buffers to use instead of fresh ones.  Nothing synchronises."""
        n, _, t, h, w = shape
        if not saved.is_cuda:
            raise I2VError("gp_backward: `saved` is a CPU tensor; libi2v_hip kernels need tensors on a HIP device (this package has no CPU fallback)")
        if saved.numel() != self.saved_bytes(n, t, h, w):
            raise I2VError(f"gp_backward: `saved` holds {saved.numel()} bytes, a saved forward on clips {tuple(shape)} holds {self.saved_bytes(n, t, h, w)}")
        need = self.gp_saved_bytes(n, t, h, w)
        if gp_saved is None:
            gp_saved = torch.empty(need, dtype=torch.uint8, device=saved.device)
        elif not gp_saved.is_cuda or gp_saved.numel() < need:
            raise I2VError(f"gp_backward: `gp_saved` must be a device buffer of at least {need} bytes")
        if l_gp is None:
            l_gp = torch.empty((), dtype=torch.float64, device=saved.device)
        ws = self._scratch(self.gp_workspace_bytes(n, t, h, w), saved.device)
        if scale_dev is None:
            _call("i2v_disc3d_gp_backward", self._h, saved.data_ptr(), saved.numel(), n, t, h, w, float(scale), gp_saved.data_ptr(), gp_saved.numel(),
                  l_gp.data_ptr(), int(bool(accumulate)), *ws, _stream())
        else:
            _require_gpu(scale_dev)
            _call("i2v_disc3d_gp_backward_dev", self._h, saved.data_ptr(), saved.numel(), n, t, h, w, float(scale), scale_dev.data_ptr(),
                  gp_saved.data_ptr(), gp_saved.numel(), l_gp.data_ptr(), int(bool(accumulate)), *ws, _stream())
        return l_gp, gp_saved

    def gp_saved_maps(self, gp_saved, shape):
        """{(kind, conv): view of ``gp_saved`` [N, T, H, W, C]} of the tangent maps (kinds DISC3D_GP_*; conv -1: the pool's, the input)."""
        n, _, t, h, w = shape
        cnt, kind, conv, dims, off = c_int32(), (c_int32 * 64)(), (c_int32 * 64)(), (c_int32 * 256)(), (c_int64 * 64)()
        _call("i2v_disc3d_gp_saved_layout", self._h, n, t, h, w, ctypes.byref(cnt), kind, conv, dims, off)
        out, flat = {}, gp_saved.view(torch.float32)
        for e in range(cnt.value):
            shp = (n, *dims[4 * e: 4 * e + 4])
            out[(kind[e], conv[e])] = flat[off[e] // 4: off[e] // 4 + int(np.prod(shp))].view(shp)
        return out


DISC3D_GP_CONV_OUT, DISC3D_GP_ACT, DISC3D_GP_POOL_OUT, DISC3D_GP_INPUT = 0, 1, 2, 3


def _gp_gn_ws(n, c, device):
    return torch.empty(int(lib().i2v_disc3d_gp_groupnorm_workspace_bytes(n, c)), dtype=torch.uint8, device=device)


def disc3d_gp_groupnorm_tangent_unit(x, xd, stats, weight, resd=None, mask=None):
    """GroupNorm's tangent over channels-last maps [N, ..., C]: x, stats of the primal -> (out, tstats float64 [N, 16, 2] = (M(xd), C(xd)))."""
    _require_gpu(x, xd, weight, resd, mask)
    n, c = x.shape[0], x.shape[-1]
    with torch.cuda.device(x.device):
        ws = _gp_gn_ws(n, c, x.device)
        out, tstats = torch.empty_like(x), torch.empty(n, 16, 2, dtype=torch.float64, device=x.device)
        _call("i2v_disc3d_gp_groupnorm_tangent_unit", x.data_ptr(), xd.data_ptr(), stats.data_ptr(), _opt(resd), _opt(mask), weight.data_ptr(), n,
              x[0].numel() // c, c, out.data_ptr(), tstats.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out, tstats


def disc3d_gp_groupnorm_dual_backward_unit(g, gd, x, xd, stats, tstats, weight, mask=None, dweight=None, dbias=None, param_grads=True):
    """-> (dx, dxd, dweight, dbias); given ``dweight`` / ``dbias`` the parameter gradients are ADDED to them."""
    _require_gpu(g, gd, x, xd, weight, mask, dweight, dbias)
    n, c = x.shape[0], x.shape[-1]
    accumulate = dweight is not None
    with torch.cuda.device(x.device):
        ws = _gp_gn_ws(n, c, x.device)
        dx, dxd = torch.empty_like(x), torch.empty_like(x)
        if param_grads and not accumulate:
            dweight, dbias = torch.empty_like(weight), torch.empty_like(weight)
        _call("i2v_disc3d_gp_groupnorm_dual_backward_unit", g.data_ptr(), gd.data_ptr(), _opt(mask), x.data_ptr(), xd.data_ptr(), stats.data_ptr(),
              tstats.data_ptr(), weight.data_ptr(), n, x[0].numel() // c, c, dx.data_ptr(), dxd.data_ptr(), _opt(dweight), _opt(dbias), int(accumulate),
              ws.data_ptr(), ws.numel(), _stream())
    return dx, dxd, dweight, dbias


def disc3d_gp_maxpool_tangent_unit(xd, argmax):
    """xd [N, T, H, W, C], argmax int32 [N, T, Ho, Wo, C] of the primal's pool -> the tangent of the pool's output."""
    _require_gpu(xd)
    n, t, h, w, c = xd.shape
    with torch.cuda.device(xd.device):
        out = torch.empty(argmax.shape, dtype=torch.float32, device=xd.device)
        _call("i2v_disc3d_gp_maxpool_tangent_unit", xd.data_ptr(), argmax.data_ptr(), n, t, h, w, c, out.data_ptr(), _stream())
    return out


def disc3d_gp_head_dual_unit(xd, weight, s=1.0):
    """xd [N, 1, 4, 4, C], weight [1, C] -> (pdot [N, 1], dx, dxd, dweight): the head's tangent and its reverse for the seed scale ``s``."""
    _require_gpu(xd, weight)
    n, c = xd.shape[0], xd.shape[-1]
    with torch.cuda.device(xd.device):
        pdot = torch.empty(n, 1, dtype=torch.float32, device=xd.device)
        dx, dxd, dw = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(weight)
        _call("i2v_disc3d_gp_head_dual_unit", xd.data_ptr(), weight.data_ptr(), float(s), n, c, pdot.data_ptr(), dx.data_ptr(), dxd.data_ptr(),
              dw.data_ptr(), _stream())
    return pdot, dx, dxd, dw


def disc3d_fmap_loss(fmap1, fmap2, metric="L1", need_grads=True, grad_scale=1.0):
    """``fmap_loss`` (loss.py:14-21) over two lists of same-layout device maps -> (out float64 [5] = (loss, the layers' own means),
    [d loss / d fmap1[i] * grad_scale] or None)."""
    if len(fmap1) != len(fmap2) or not 1 <= len(fmap1) <= 4 or metric not in FMAP_METRICS:
        raise I2VError(f"disc3d_fmap_loss: {len(fmap1)} against {len(fmap2)} maps (1..4), metric {metric!r} ('L1' or 'L2')")
    _require_gpu(*fmap1, *fmap2)
    for a, b in zip(fmap1, fmap2):
        if a.shape != b.shape:
            raise I2VError(f"disc3d_fmap_loss: map {tuple(a.shape)} against {tuple(b.shape)}")
    dev, nl = fmap1[0].device, len(fmap1)
    with torch.cuda.device(dev):
        out = torch.empty(5, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib().i2v_disc3d_fmap_loss_workspace_bytes()), dtype=torch.uint8, device=dev)
        grads = [torch.empty_like(a) for a in fmap1] if need_grads else None
        _call("i2v_disc3d_fmap_loss", _ptr_array(fmap1, nl), _ptr_array(fmap2, nl), (c_int64 * nl)(*[a.numel() for a in fmap1]), nl, FMAP_METRICS[metric],
              float(grad_scale), out.data_ptr(), _ptr_array(grads, nl), ws.data_ptr(), ws.numel(), _stream())
    return out, grads


def disc3d_sumsq(x):
    """x [N, ...] -> float64 [N]: the sum of squares of each sample."""
    _require_gpu(x)
    with torch.cuda.device(x.device):
        out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        _call("i2v_disc3d_sumsq", x.data_ptr(), x.shape[0], x[0].numel(), out.data_ptr(), _stream())
    return out


def disc3d_wgrad_plan(cout, cin, positions, taps=27):
    """(slices, slice_len) of the weight gradient's position split: a pure host function of the shape."""
    s, l = c_int32(), c_int32()
    _call("i2v_disc3d_wgrad_plan", int(cout), int(cin), int(taps), int(positions), ctypes.byref(s), ctypes.byref(l))
    return s.value, l.value


def disc3d_out_extent(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _d3_geom(x, weight):
    n, ti, hi, wi, cs = x.shape
    cout, cin, kt, kh, kw = weight.shape
    stem = (kh, kw) == (7, 7)
    if cs != (4 if cin == 3 else cin) or kt != 3 or (kh, kw) not in ((3, 3), (7, 7)):
        raise I2VError(f"temporal discriminator unit: map {tuple(x.shape)} against weight {tuple(weight.shape)}")
    return n, ti, hi, wi, cin, cout, int(stem)


def _d3_ws(n, ti, hi, wi, cin, cout, stem, device):
    return torch.empty(int(lib().i2v_disc3d_unit_workspace_bytes(n, ti, hi, wi, cin, cout, stem)), dtype=torch.uint8, device=device)


def disc3d_conv_unit(x, weight, stride_t=1, stride_s=1):
    """x [N, T, H, W, C] channels-last (C = 4 for cin 3), weight [Cout, Cin, 3, k, k] -> [N, To, Ho, Wo, Cout]."""
    _require_gpu(x, weight)
    n, ti, hi, wi, cin, cout, stem = _d3_geom(x, weight)
    k = weight.shape[-1]
    with torch.cuda.device(x.device):
        ws = _d3_ws(n, ti, hi, wi, cin, cout, stem, x.device)
        out = torch.empty(n, disc3d_out_extent(ti, 3, stride_t), disc3d_out_extent(hi, k, stride_s), disc3d_out_extent(wi, k, stride_s), cout,
                          dtype=torch.float32, device=x.device)
        _call("i2v_disc3d_conv_unit", x.data_ptr(), weight.data_ptr(), n, ti, hi, wi, cin, cout, stem, stride_t, stride_s, out.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    return out


def disc3d_dgrad_unit(g, weight, in_thw, act=None, add=None, add_mask=None, stride_t=1, stride_s=1, frames=False):
    """g [N, To, Ho, Wo, Cout] -> the gradient at the conv's input [N, T, H, W, Cin] (cin 3: 4 channels, or [N, 3, T, H, W] with ``frames``)."""
    _require_gpu(g, weight, act, add, add_mask)
    n, (ti, hi, wi), (cout, cin) = g.shape[0], in_thw, weight.shape[:2]
    stem = int(weight.shape[-1] == 7)
    with torch.cuda.device(g.device):
        ws = _d3_ws(n, ti, hi, wi, cin, cout, stem, g.device)
        out = torch.empty((n, 3, ti, hi, wi) if frames else (n, ti, hi, wi, 4 if cin == 3 else cin), dtype=torch.float32, device=g.device)
        _call("i2v_disc3d_dgrad_unit", g.data_ptr(), weight.data_ptr(), _opt(act), _opt(add), _opt(add_mask), n, ti, hi, wi, cin, cout, stem, stride_t,
              stride_s, out.data_ptr(), int(bool(frames)), ws.data_ptr(), ws.numel(), _stream())
    return out


def disc3d_wgrad_unit(g, x, weight, act=None, u=None, v=None, sigma=None, stride_t=1, stride_s=1, dweight=None):
    """-> dweight [Cout, Cin, 3, k, k]; given ``dweight`` the result is ADDED to it."""
    _require_gpu(g, x, weight, act, u, v, sigma, dweight)
    n, ti, hi, wi, cin, cout, stem = _d3_geom(x, weight)
    accumulate = dweight is not None
    with torch.cuda.device(g.device):
        ws = _d3_ws(n, ti, hi, wi, cin, cout, stem, g.device)
        if not accumulate:
            dweight = torch.empty_like(weight)
        _call("i2v_disc3d_wgrad_unit", g.data_ptr(), _opt(act), x.data_ptr(), weight.data_ptr(), _opt(u), _opt(v), _opt(sigma), n, ti, hi, wi, cin, cout,
              stem, stride_t, stride_s, int(accumulate), dweight.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return dweight


def _gn_ws(n, c, device):
    return torch.empty(int(lib().i2v_disc3d_groupnorm_workspace_bytes(n, c)), dtype=torch.uint8, device=device)


def disc3d_groupnorm_unit(x, weight, bias, res=None, relu=False):
    """GroupNorm(16) over x [N, ..., C] channels-last -> (out, stats float64 [N, 16, 2] = (mean, rstd))."""
    _require_gpu(x, weight, bias, res)
    n, c = x.shape[0], x.shape[-1]
    with torch.cuda.device(x.device):
        ws = _gn_ws(n, c, x.device)
        out, stats = torch.empty_like(x), torch.empty(n, 16, 2, dtype=torch.float64, device=x.device)
        _call("i2v_disc3d_groupnorm_unit", x.data_ptr(), _opt(res), weight.data_ptr(), bias.data_ptr(), n, x[0].numel() // c, c, int(bool(relu)),
              out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out, stats


def disc3d_groupnorm_backward_unit(g, x, stats, weight, mask=None, dweight=None, dbias=None, param_grads=True):
    """-> (dx, dweight, dbias); given ``dweight`` / ``dbias`` the parameter gradients are ADDED to them."""
    _require_gpu(g, x, weight, mask, dweight, dbias)
    n, c = x.shape[0], x.shape[-1]
    accumulate = dweight is not None
    with torch.cuda.device(x.device):
        ws = _gn_ws(n, c, x.device)
        dx = torch.empty_like(x)
        if param_grads and not accumulate:
            dweight, dbias = torch.empty_like(weight), torch.empty_like(weight)
        _call("i2v_disc3d_groupnorm_backward_unit", g.data_ptr(), _opt(mask), x.data_ptr(), stats.data_ptr(), weight.data_ptr(), n, x[0].numel() // c, c,
              dx.data_ptr(), _opt(dweight), _opt(dbias), int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return dx, dweight, dbias


def disc3d_maxpool_unit(x):
    """MaxPool3d(3, stride (1, 2, 2), pad 1) on x [N, T, H, W, C] -> (out, argmax int32)."""
    _require_gpu(x)
    n, t, h, w, c = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty(n, t, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=torch.float32, device=x.device)
        arg = torch.empty(out.shape, dtype=torch.int32, device=x.device)
        _call("i2v_disc3d_maxpool_unit", x.data_ptr(), n, t, h, w, c, out.data_ptr(), arg.data_ptr(), _stream())
    return out, arg


def disc3d_maxpool_backward_unit(g, argmax, in_shape):
    _require_gpu(g)
    n, t, h, w, c = in_shape
    with torch.cuda.device(g.device):
        dx = torch.empty(in_shape, dtype=torch.float32, device=g.device)
        _call("i2v_disc3d_maxpool_backward_unit", g.data_ptr(), argmax.data_ptr(), n, t, h, w, c, dx.data_ptr(), _stream())
    return dx


def disc3d_head_unit(x, weight, g=None):
    """x [N, 1, 4, 4, C], weight [1, C] -> pred [N, 1]; with g [N, 1] also (dx, dweight)."""
    _require_gpu(x, weight, g)
    n, c = x.shape[0], x.shape[-1]
    with torch.cuda.device(x.device):
        pred = torch.empty(n, 1, dtype=torch.float32, device=x.device)
        dx, dw = (torch.empty_like(x), torch.empty_like(weight)) if g is not None else (None, None)
        _call("i2v_disc3d_head_unit", x.data_ptr(), weight.data_ptr(), _opt(g), n, c, pred.data_ptr(), _opt(dx), _opt(dw), _stream())
    return pred if g is None else (pred, dx, dw)


# ---------------------------------------------------------------------------------------------------------------- motion encoder, training path
ENC3D_TRAIN_SAVE = 1
ENC3D_TRAIN_CONV_OUT, ENC3D_TRAIN_ACT = 0, 1


class NativeEnc3DTrain(_Res3DHandle):
    """Handle for ``i2v_enc3d_train_*`` (include/i2v_hip_enc3d_train.h): resnet3D.Encoder forward and backward with the posterior head and
    the KL gradient.  It packs nothing on the host: ``bind`` hands over the DEVICE pointers of the module's parameters (read in place, so
    an optimiser step is seen by the next call) and ``bind_grads`` those of their gradient tensors."""
    _PREFIX, _NAME = "i2v_enc3d_train", "motion encoder"

    def __init__(self, z_dim, channels, stride_s, stride_t, use_max_pool=False, device=None):
        if len(channels) != 5 or len(stride_s) != 4 or len(stride_t) != 4:
            raise I2VError(f"motion encoder: {len(channels)} widths with {len(stride_s)} / {len(stride_t)} strides (5 and 4 are built)")
        cfg = Enc3dTrainCfg(int(z_dim), (c_int32 * 5)(*map(int, channels)), (c_int32 * 4)(*map(int, stride_s)), (c_int32 * 4)(*map(int, stride_t)),
                            int(bool(use_max_pool)))
        self._create(device, ctypes.byref(cfg))
        self.z_dim = int(z_dim)

    def out_shape(self, t, h, w):
        """(t, h, w, c) of the trunk's last map; raises with the map in the message unless it is [1, 4, 4]."""
        s = (c_int32 * 4)()
        _call("i2v_enc3d_train_out_shape", self._h, int(t), int(h), int(w), s)
        return tuple(s)

    @_on_device
    def forward(self, x, eps=None, save=False):
        """x [N, 3, T, H, W], eps [N, z] or None -> (sample or None, mu, logvar, saved or None)."""
        _require_gpu(x, eps)
        n, t, h, w = self._shape(x)
        if eps is not None and tuple(eps.shape) != (n, self.z_dim):
            raise I2VError(f"motion encoder: expected eps [{n},{self.z_dim}], got {tuple(eps.shape)}")
        self.out_shape(t, h, w)
        ws = self._scratch(self.workspace_bytes(n, t, h, w), x.device)
        saved = torch.empty(self.saved_bytes(n, t, h, w), dtype=torch.uint8, device=x.device) if save else None
        mu = torch.empty(n, self.z_dim, dtype=torch.float32, device=x.device)
        logvar = torch.empty_like(mu)
        sample = torch.empty_like(mu) if eps is not None else None
        _call("i2v_enc3d_train_forward", self._h, x.data_ptr(), _opt(eps), n, t, h, w, ENC3D_TRAIN_SAVE if save else 0, _opt(sample), mu.data_ptr(),
              logvar.data_ptr(), _opt(saved), 0 if saved is None else saved.numel(), *ws, _stream())
        return sample, mu, logvar, saved

    @_on_device
    def backward(self, d_sample, d_mu, d_logvar, saved, shape, kl_scale=0.0, need_dx=True, param_grads=True, accumulate=False):
        """``shape``: the (N, 3, T, H, W) of the forward's input; the upstream gradients [N, z] or None -> d_x [N, 3, T, H, W] or None; the
        parameter gradients go to the bound gradient tensors, written or (``accumulate``) added."""
        _require_gpu(d_sample, d_mu, d_logvar)
        n, _, t, h, w = shape
        ws = self._scratch(self.workspace_bytes(n, t, h, w), saved.device)
        dx = torch.empty(n, 3, t, h, w, dtype=torch.float32, device=saved.device) if need_dx else None
        _call("i2v_enc3d_train_backward", self._h, _opt(d_sample), _opt(d_mu), _opt(d_logvar), float(kl_scale), saved.data_ptr(), saved.numel(), n, t, h,
              w, _opt(dx), int(bool(param_grads)), int(bool(accumulate)), *ws, _stream())
        return dx


def enc3d_kl_backward(mu, logvar, scale=1.0):
    """The gradient of ``scale * KL(mu, logvar)`` (loss.py:10-12) -> (d_mu, d_logvar) fp32 [N, z]."""
    _require_gpu(mu, logvar)
    n, z = mu.shape
    with torch.cuda.device(mu.device):
        d_mu, d_lv = torch.empty_like(mu), torch.empty_like(logvar)
        _call("i2v_enc3d_kl_backward", mu.data_ptr(), logvar.data_ptr(), n, z, float(scale), d_mu.data_ptr(), d_lv.data_ptr(), _stream())
    return d_mu, d_lv


def _enc3d_head_ws(n, c, z, device):
    return torch.empty(int(lib().i2v_enc3d_head_workspace_bytes(n, c, z)), dtype=torch.uint8, device=device)


def enc3d_head_forward_unit(emb, w_mu, b_mu, w_var, b_var, eps=None):
    """emb [N, 16, C] channels-last, weights [z, C, 4, 4], biases [z] -> (sample or None, mu, logvar) [N, z]."""
    _require_gpu(emb, w_mu, b_mu, w_var, b_var, eps)
    n, c, z = emb.shape[0], emb.shape[-1], w_mu.shape[0]
    with torch.cuda.device(emb.device):
        ws = _enc3d_head_ws(n, c, z, emb.device)
        mu = torch.empty(n, z, dtype=torch.float32, device=emb.device)
        logvar = torch.empty_like(mu)
        sample = torch.empty_like(mu) if eps is not None else None
        _call("i2v_enc3d_head_forward_unit", emb.data_ptr(), w_mu.data_ptr(), b_mu.data_ptr(), w_var.data_ptr(), b_var.data_ptr(), _opt(eps), n, c, z,
              _opt(sample), mu.data_ptr(), logvar.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return sample, mu, logvar


def enc3d_head_backward_unit(emb, w_mu, w_var, mu, logvar, eps=None, d_sample=None, d_mu=None, d_logvar=None, kl_scale=0.0, param_grads=True,
                             into=None):
    """-> (d_emb [N, 16, C], dw_mu, db_mu, dw_var, db_var); given ``into`` (those four tensors) the parameter gradients are ADDED to them."""
    _require_gpu(emb, w_mu, w_var, mu, logvar, eps, d_sample, d_mu, d_logvar)
    n, c, z = emb.shape[0], emb.shape[-1], w_mu.shape[0]
    with torch.cuda.device(emb.device):
        ws = _enc3d_head_ws(n, c, z, emb.device)
        d_emb = torch.empty_like(emb)
        grads = into
        if param_grads and into is None:
            grads = (torch.empty_like(w_mu), torch.empty(z, dtype=torch.float32, device=emb.device), torch.empty_like(w_var),
                     torch.empty(z, dtype=torch.float32, device=emb.device))
        g = grads if param_grads else (None,) * 4
        _call("i2v_enc3d_head_backward_unit", emb.data_ptr(), w_mu.data_ptr(), w_var.data_ptr(), mu.data_ptr(), logvar.data_ptr(), _opt(eps),
              _opt(d_sample), _opt(d_mu), _opt(d_logvar), float(kl_scale), n, c, z, d_emb.data_ptr(), *[_opt(t) for t in g], int(into is not None),
              ws.data_ptr(), ws.numel(), _stream())
    return (d_emb, *g)


# ---------------------------------------------------------------------------------------------------------------- GeneratorBlock, training path
GBLOCK_TRAIN_SAVE, GBLOCK_TRAIN_TRAIN = 1, 2
GBLOCK_TRAIN_SPADE, GBLOCK_TRAIN_ADAIN = 0, 1


class NativeGBlockTrain(_BoundHandle):
    """Handle for ``i2v_gblock_train_*`` (include/i2v_hip_gblock_train.h): one GeneratorBlock forward and backward in exact fp32.  It packs
    nothing on the host: ``bind`` hands over the DEVICE pointers of the module's parameters and spectral-norm buffers (read in place, so an
    optimiser step is seen by the next call; ``weight_u`` / ``weight_v`` are iterated in place) and ``bind_grads`` those of the gradients."""
    _PREFIX = "i2v_gblock_train"

    def __init__(self, n_in, n_out, z_dim, spectral_norm=True, device=None):
        self._create(device, int(n_in), int(n_out), int(z_dim), int(bool(spectral_norm)))
        self.n_in, self.n_out, self.n_mid, self.z_dim = int(n_in), int(n_out), min(int(n_in), int(n_out)), int(z_dim)

    def _geom(self, shape, img_shape):
        B, _, T, H, W = shape
        return B, T, H, W, int(img_shape[2]), int(img_shape[3])

    def saved_bytes(self, *geom):
        return int(lib().i2v_gblock_train_saved_bytes(self._h, *geom))

    def workspace_bytes(self, *geom):
        return int(lib().i2v_gblock_train_workspace_bytes(self._h, *geom))

    @_on_device
    def forward(self, x, z, img, train=False, save=False):
        """x [B, n_in, T, H, W], z [B, z_dim], img [B, 3, h, w] -> (out [B, n_out, T, H, W], saved or None)."""
        _require_gpu(x, z, img)
        if x.dim() != 5 or x.shape[1] != self.n_in:
            raise I2VError(f"GeneratorBlock: expected x [B,{self.n_in},T,H,W], got {tuple(x.shape)}")
        B = x.shape[0]
        if z.shape != (B, self.z_dim) or img.dim() != 4 or img.shape[:2] != (B, 3):
            raise I2VError(f"GeneratorBlock: expected z [B,{self.z_dim}] and img [B,3,h,w], got {tuple(z.shape)}, {tuple(img.shape)}")
        geom = self._geom(x.shape, img.shape)
        ws = self._scratch(self.workspace_bytes(*geom), x.device)
        saved = torch.empty(self.saved_bytes(*geom), dtype=torch.uint8, device=x.device) if save else None
        out = torch.empty(B, self.n_out, *x.shape[2:], dtype=torch.float32, device=x.device)
        flags = (GBLOCK_TRAIN_SAVE if save else 0) | (GBLOCK_TRAIN_TRAIN if train else 0)
        _call("i2v_gblock_train_forward", self._h, x.data_ptr(), z.data_ptr(), img.data_ptr(), *geom, flags, out.data_ptr(), _opt(saved),
              0 if saved is None else saved.numel(), *ws, _stream())
        return out, saved

    @_on_device
    def backward(self, g_out, z, saved, shape, img_shape, need_dx=True, need_dz=True, param_grads=True, accumulate=False):
        """``shape`` / ``img_shape``: those of the forward's x and img -> (dx or None, dz or None); the parameter gradients go to the bound
        gradient tensors, written or (``accumulate``) added."""
        _require_gpu(g_out, z)
        geom = self._geom(shape, img_shape)
        ws = self._scratch(self.workspace_bytes(*geom), saved.device)
        dx = torch.empty(shape, dtype=torch.float32, device=saved.device) if need_dx else None
        dz = torch.empty(shape[0], self.z_dim, dtype=torch.float32, device=saved.device) if need_dz else None
        _call("i2v_gblock_train_backward", self._h, g_out.data_ptr(), z.data_ptr(), saved.data_ptr(), saved.numel(), *geom, _opt(dx), _opt(dz),
              int(bool(param_grads)), int(bool(accumulate)), *ws, _stream())
        return dx, dz


def _gbt_ws(batch, rows, c, device):
    return torch.empty(int(lib().i2v_gblock_train_unit_workspace_bytes(int(batch), int(rows), int(c))), dtype=torch.uint8, device=device)


def gblock_train_modnorm_backward_unit(mode, g, act, x, mod, add=None, want_dx=True, want_maps=True):
    """g, act, x [B, T, H, W, C] channels-last.  Spade (mode 0): mod = gamma [B, H, W, C] -> (dx, dgamma, dbeta [B, H, W, C]); ADAIN (mode 1):
    mod = lin [B, 2 C] -> (dx, d_lin [B, 2 C], None).  What is not wanted comes back as None."""
    _require_gpu(g, act, x, mod, add)
    B, T, H, W, C = x.shape
    with torch.cuda.device(x.device):
        ws = _gbt_ws(B, x.numel() // C, C, x.device)
        dx = torch.empty_like(x) if want_dx else None
        dgamma = torch.empty_like(mod) if want_maps else None
        dbeta = torch.empty_like(mod) if want_maps and mode == GBLOCK_TRAIN_SPADE else None
        _call("i2v_gblock_train_modnorm_backward_unit", int(mode), g.data_ptr(), act.data_ptr(), x.data_ptr(), mod.data_ptr(), B, T, H, W, C, _opt(add),
              _opt(dx), _opt(dgamma), _opt(dbeta), ws.data_ptr(), ws.numel(), _stream())
    return dx, dgamma, dbeta


def gblock_train_pointwise_unit(a, w, add=None):
    """a [..., K] channels-last, w [N, K] -> a . w^T (+ add) [..., N]."""
    _require_gpu(a, w, add)
    k, n = a.shape[-1], w.shape[0]
    with torch.cuda.device(a.device):
        out = torch.empty(*a.shape[:-1], n, dtype=torch.float32, device=a.device)
        _call("i2v_gblock_train_pointwise_unit", a.data_ptr(), w.data_ptr(), _opt(add), a.numel() // k, k, n, out.data_ptr(), _stream())
    return out


def gblock_train_pointwise_wgrad_unit(g, x, w, u=None, v=None, sigma=None, dweight=None):
    """g [..., Cout], x [..., Cin], w [Cout, Cin] -> dweight; given ``dweight`` the result is ADDED to it."""
    _require_gpu(g, x, w, u, v, sigma, dweight)
    cout, cin = w.shape
    accumulate = dweight is not None
    with torch.cuda.device(g.device):
        ws = _gbt_ws(1, g.numel() // cout, max(cout, cin), g.device)
        if not accumulate:
            dweight = torch.empty_like(w)
        _call("i2v_gblock_train_pointwise_wgrad_unit", g.data_ptr(), x.data_ptr(), w.data_ptr(), _opt(u), _opt(v), _opt(sigma), g.numel() // cout, cout,
              cin, int(accumulate), dweight.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return dweight


def gblock_train_bias_grad_unit(g, dbias=None):
    """g [..., C] -> the float64 sum over the rows, rounded once; given ``dbias`` the result is ADDED to it."""
    _require_gpu(g, dbias)
    c = g.shape[-1]
    accumulate = dbias is not None
    with torch.cuda.device(g.device):
        ws = _gbt_ws(1, g.numel() // c, c, g.device)
        if not accumulate:
            dbias = torch.empty(c, dtype=torch.float32, device=g.device)
        _call("i2v_gblock_train_bias_grad_unit", g.data_ptr(), g.numel() // c, c, int(accumulate), dbias.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return dbias


def gblock_train_linear_backward_unit(d_lin, z, w, want=(True, True, True)):
    """d_lin [B, J], z [B, K], w [J, K] -> (dw, db, dz), each None where ``want`` says so."""
    _require_gpu(d_lin, z, w)
    (B, J), K = d_lin.shape, z.shape[1]
    with torch.cuda.device(z.device):
        dw = torch.empty_like(w) if want[0] else None
        db = torch.empty(J, dtype=torch.float32, device=z.device) if want[1] else None
        dz = torch.empty_like(z) if want[2] else None
        _call("i2v_gblock_train_linear_backward_unit", d_lin.data_ptr(), z.data_ptr(), w.data_ptr(), B, J, K, 0, _opt(dw), _opt(db), _opt(dz), _stream())
    return dw, db, dz


def gblock_train_conv2d_unit(x, w, g=None, want=(True, True, True)):
    """x [B, H, W, Cin] channels-last (4 channels for Cin = 3), w [Cout, Cin, 3, 3], g [B, H, W, Cout] -> (y, dx, dw), None where unwanted."""
    _require_gpu(x, w, g)
    B, H, W, _ = x.shape
    cout, cin = w.shape[:2]
    with torch.cuda.device(x.device):
        ws = _gbt_ws(B, B * H * W, max(cout, cin, 16), x.device)
        y = torch.empty(B, H, W, cout, dtype=torch.float32, device=x.device) if want[0] else None
        dx = torch.empty(B, H, W, cin, dtype=torch.float32, device=x.device) if want[1] and g is not None else None
        dw = torch.empty_like(w) if want[2] and g is not None else None
        _call("i2v_gblock_train_conv2d_unit", x.data_ptr(), w.data_ptr(), _opt(g), B, H, W, cin, cout, _opt(y), _opt(dx), _opt(dw), ws.data_ptr(),
              ws.numel(), _stream())
    return y, dx, dw


# ---------------------------------------------------------------------------------------------------------------- Generator, training path
GEN_TRAIN_SAVE = 1
UPSAMPLE_FACTORS = (1, 2, 4)


class NativeGenTrain(_BoundHandle):
    """Handle for ``i2v_gen_train_*`` (include/i2v_hip_gen_train.h): what the Generator's training path runs between and around its six
    GeneratorBlocks -- ``fc`` and the image head ``tanh(conv_img(lrelu(x)))``, forward and backward in exact fp32.  It packs nothing on the
    host: ``bind`` hands over the DEVICE pointers of ``fc.{weight,bias}`` and ``conv_img.{weight,bias}`` (read in place, so an optimiser step
    is seen by the next call) and ``bind_grads`` those of their gradients."""
    _PREFIX = "i2v_gen_train"

    def __init__(self, channel_factor, z_dim, device=None):
        self._create(device, int(channel_factor), int(z_dim))
        self.nf, self.z_dim = int(channel_factor), int(z_dim)

    @_on_device
    def fc_forward(self, z):
        """z [B, z_dim] -> [B, 256 nf] (the reshape to [B, 16 nf, 1, 4, 4] is a view)."""
        _require_gpu(z)
        if z.dim() != 2 or z.shape[1] != self.z_dim:
            raise I2VError(f"Generator: expected motion [B,{self.z_dim}], got {tuple(z.shape)}")
        out = torch.empty(z.shape[0], 256 * self.nf, dtype=torch.float32, device=z.device)
        _call("i2v_gen_train_fc_forward", self._h, z.data_ptr(), z.shape[0], out.data_ptr(), _stream())
        return out

    @_on_device
    def fc_backward(self, g_out, z, need_dz=True, param_grads=True, accumulate=False):
        """g_out [B, 256 nf] -> dz [B, z_dim] or None; the parameter gradients go to the bound gradient tensors."""
        _require_gpu(g_out, z)
        B = z.shape[0]
        ws = self._scratch(int(lib().i2v_gen_train_fc_workspace_bytes(B, 256 * self.nf, self.z_dim)), z.device)
        dz = torch.empty(B, self.z_dim, dtype=torch.float32, device=z.device) if need_dz else None
        _call("i2v_gen_train_fc_backward", self._h, g_out.data_ptr(), z.data_ptr(), B, _opt(dz), int(bool(param_grads)), int(bool(accumulate)), *ws,
              _stream())
        return dz

    def _head_geom(self, shape):
        B, C, T, H, W = shape
        if C != self.nf:
            raise I2VError(f"Generator: expected x [B,{self.nf},T,H,W] in front of conv_img, got {tuple(shape)}")
        return int(B), int(T), int(H), int(W)

    @_on_device
    def head_forward(self, x, save=False):
        """x [B, nf, T, H, W] -> (frames [B, T, 3, H, W], saved or None)."""
        _require_gpu(x)
        geom = self._head_geom(x.shape)
        ws = self._scratch(int(lib().i2v_gen_train_head_workspace_bytes(self.nf, *geom)), x.device)
        saved = torch.empty(int(lib().i2v_gen_train_head_saved_bytes(self.nf, *geom)), dtype=torch.uint8, device=x.device) if save else None
        B, T, H, W = geom
        out = torch.empty(B, T, 3, H, W, dtype=torch.float32, device=x.device)
        _call("i2v_gen_train_head_forward", self._h, x.data_ptr(), *geom, GEN_TRAIN_SAVE if save else 0, out.data_ptr(), _opt(saved),
              0 if saved is None else saved.numel(), *ws, _stream())
        return out, saved

    @_on_device
    def head_backward(self, g_out, saved, shape, need_dx=True, param_grads=True, accumulate=False):
        """``shape``: that of the forward's x -> dx or None; the parameter gradients go to the bound gradient tensors."""
        _require_gpu(g_out)
        geom = self._head_geom(shape)
        ws = self._scratch(int(lib().i2v_gen_train_head_workspace_bytes(self.nf, *geom)), saved.device)
        dx = torch.empty(tuple(shape), dtype=torch.float32, device=saved.device) if need_dx else None
        _call("i2v_gen_train_head_backward", self._h, g_out.data_ptr(), saved.data_ptr(), saved.numel(), *geom, _opt(dx), int(bool(param_grads)),
              int(bool(accumulate)), *ws, _stream())
        return dx


def gen_train_fc_slices(j):
    """The slices of the ``j`` rows that the fc backward's dz adds in slice order."""
    return int(lib().i2v_gen_train_fc_slices(int(j)))


def _up_factors(ut, us):
    if int(ut) not in UPSAMPLE_FACTORS or int(us) not in UPSAMPLE_FACTORS:
        raise I2VError(f"nearest up-sampling by ({ut}, {us}, {us}): each factor must be one of {UPSAMPLE_FACTORS}")
    return int(ut), int(us)


def gen_train_upsample(x, ut, us):
    """x [B, C, T, H, W] -> [B, C, ut T, us H, us W], ``F.interpolate(x, scale_factor=(ut, us, us))`` bit for bit."""
    _require_gpu(x)
    ut, us = _up_factors(ut, us)
    B, C, T, H, W = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty(B, C, T * ut, H * us, W * us, dtype=torch.float32, device=x.device)
        _call("i2v_gen_train_upsample_forward", x.data_ptr(), B * C, T, H, W, ut, us, out.data_ptr(), _stream())
    return out


def gen_train_upsample_backward(g, ut, us):
    """g [B, C, ut T, us H, us W] -> [B, C, T, H, W]: the box sums in fp32 in (dt, dh, dw) order."""
    _require_gpu(g)
    ut, us = _up_factors(ut, us)
    B, C, To, Ho, Wo = g.shape
    if To % ut or Ho % us or Wo % us:
        raise I2VError(f"up-sampling backward: {tuple(g.shape)} is not a map up-sampled by ({ut}, {us}, {us})")
    with torch.cuda.device(g.device):
        dx = torch.empty(B, C, To // ut, Ho // us, Wo // us, dtype=torch.float32, device=g.device)
        _call("i2v_gen_train_upsample_backward", g.data_ptr(), B * C, To // ut, Ho // us, Wo // us, ut, us, dx.data_ptr(), _stream())
    return dx


def gen_train_fc_forward_unit(z, w, bias):
    """z [B, K], w [J, K], bias [J] -> [B, J]."""
    _require_gpu(z, w, bias)
    with torch.cuda.device(z.device):
        out = torch.empty(z.shape[0], w.shape[0], dtype=torch.float32, device=z.device)
        _call("i2v_gen_train_fc_forward_unit", z.data_ptr(), w.data_ptr(), bias.data_ptr(), z.shape[0], w.shape[0], w.shape[1], out.data_ptr(), _stream())
    return out


def gen_train_fc_backward_unit(g, z, w, want_params=True, want_dz=True):
    """g [B, J], z [B, K], w [J, K] -> (dw, db, dz), None where unwanted."""
    _require_gpu(g, z, w)
    (B, J), K = g.shape, z.shape[1]
    with torch.cuda.device(z.device):
        ws = torch.empty(int(lib().i2v_gen_train_fc_workspace_bytes(B, J, K)), dtype=torch.uint8, device=z.device)
        dw = torch.empty_like(w) if want_params else None
        db = torch.empty(J, dtype=torch.float32, device=z.device) if want_params else None
        dz = torch.empty_like(z) if want_dz else None
        _call("i2v_gen_train_fc_backward_unit", g.data_ptr(), z.data_ptr(), w.data_ptr(), B, J, K, 0, _opt(dw), _opt(db), _opt(dz), ws.data_ptr(),
              ws.numel(), _stream())
    return dw, db, dz


def gen_train_head_forward_unit(x, w, bias, save=True):
    """x [B, nf, T, H, W], w [3, nf, 3, 3, 3], bias [3] -> (frames [B, T, 3, H, W], saved or None)."""
    _require_gpu(x, w, bias)
    B, nf, T, H, W = x.shape
    with torch.cuda.device(x.device):
        ws = torch.empty(int(lib().i2v_gen_train_head_workspace_bytes(nf, B, T, H, W)), dtype=torch.uint8, device=x.device)
        saved = torch.empty(int(lib().i2v_gen_train_head_saved_bytes(nf, B, T, H, W)), dtype=torch.uint8, device=x.device) if save else None
        out = torch.empty(B, T, 3, H, W, dtype=torch.float32, device=x.device)
        _call("i2v_gen_train_head_forward_unit", x.data_ptr(), w.data_ptr(), bias.data_ptr(), nf, B, T, H, W, out.data_ptr(), _opt(saved),
              0 if saved is None else saved.numel(), ws.data_ptr(), ws.numel(), _stream())
    return out, saved


def gen_train_head_backward_unit(g, saved, w, shape, want_dx=True, want_params=True):
    """g [B, T, 3, H, W], ``saved`` of the forward, ``shape`` that of its x -> (dx, dw, db), None where unwanted."""
    _require_gpu(g, w)
    B, nf, T, H, W = shape
    with torch.cuda.device(g.device):
        ws = torch.empty(int(lib().i2v_gen_train_head_workspace_bytes(nf, B, T, H, W)), dtype=torch.uint8, device=g.device)
        dx = torch.empty(tuple(shape), dtype=torch.float32, device=g.device) if want_dx else None
        dw = torch.empty_like(w) if want_params else None
        db = torch.empty(3, dtype=torch.float32, device=g.device) if want_params else None
        _call("i2v_gen_train_head_backward_unit", g.data_ptr(), saved.data_ptr(), saved.numel(), w.data_ptr(), nf, B, T, H, W, 0, _opt(dx), _opt(dw),
              _opt(db), ws.data_ptr(), ws.numel(), _stream())
    return dx, dw, db
