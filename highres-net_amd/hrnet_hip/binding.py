"""ctypes binding of libhrnet_hip.so (C ABI: include/hrnet_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory (`tensor.data_ptr()`), the current HIP stream and, for
multi-GPU, `torch.distributed`.  All arithmetic happens in the hand-written gfx950 kernels of the library.
There is NO fallback: if the library is missing or a tensor is not on a ROCm device, these functions raise.
"""
import ctypes
import os
import threading

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment
from .resample import check_scale

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HRNET_HIP_LIB") or os.path.join(_HERE, "libhrnet_hip.so")   # override: A/B-testing a build

F32, BF16, BF16X3 = 0, 1, 2
MAX_RES_LAYERS = 8
_DT_TORCH = {F32: torch.float32, BF16: torch.bfloat16, BF16X3: torch.bfloat16}     # BF16X3: two bf16 planes (hi, lo), planes first


def planes_to_float(t, dtype):
    """A stage tensor as float32: bf16x3 stage tensors are (2, ...) bf16 pairs of planes, value = hi + lo."""
    return t[0].float() + t[1].float() if dtype == BF16X3 else t.float()


def float_to_planes(x, dtype):
    """float32 -> the stage tensor of `dtype` (bf16x3: hi = bf16(x), lo = bf16(x - hi), stacked planes first)."""
    if dtype == BF16X3:
        hi = x.to(torch.bfloat16)
        return torch.stack([hi, (x - hi.float()).to(torch.bfloat16)]).contiguous()
    return x.to(_DT_TORCH[dtype]).contiguous()
_fp = ctypes.POINTER(ctypes.c_float)


class HrnetParams(ctypes.Structure):
    _fields_ = [
        ("num_layers", ctypes.c_int),
        ("enc_init_w", ctypes.c_void_p), ("enc_init_b", ctypes.c_void_p), ("enc_init_a", ctypes.c_void_p),
        ("enc_res_w", ctypes.c_void_p * (2 * MAX_RES_LAYERS)),
        ("enc_res_b", ctypes.c_void_p * (2 * MAX_RES_LAYERS)),
        ("enc_res_a", ctypes.c_void_p * (2 * MAX_RES_LAYERS)),
        ("enc_final_w", ctypes.c_void_p), ("enc_final_b", ctypes.c_void_p),
        ("fuse_res_w", ctypes.c_void_p * 2), ("fuse_res_b", ctypes.c_void_p * 2), ("fuse_res_a", ctypes.c_void_p * 2),
        ("fuse_out_w", ctypes.c_void_p), ("fuse_out_b", ctypes.c_void_p), ("fuse_out_a", ctypes.c_void_p),
        ("dec_w", ctypes.c_void_p), ("dec_b", ctypes.c_void_p), ("dec_a", ctypes.c_void_p),
        ("fin_w", ctypes.c_void_p), ("fin_b", ctypes.c_void_p),
    ]


class ShiftnetParams(ctypes.Structure):
    _fields_ = [
        ("conv_w", ctypes.c_void_p * 8), ("conv_b", ctypes.c_void_p * 8),
        ("bn_g", ctypes.c_void_p * 8), ("bn_b", ctypes.c_void_p * 8),
        ("bn_rm", ctypes.c_void_p * 8), ("bn_rv", ctypes.c_void_p * 8),
        ("fc1_w", ctypes.c_void_p), ("fc1_b", ctypes.c_void_p), ("fc2_w", ctypes.c_void_p),
    ]


# name -> (restype, argtypes); must list every symbol include/hrnet_hip.h declares (checked by tests/test_abi.py)
_c = ctypes
SIGNATURES = {
    "hrn_version": (_c.c_int, []),
    "hrn_last_error": (_c.c_char_p, []),
    "hrn_hrnet_packed_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "hrn_hrnet_pack": (_c.c_int, [_c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "hrn_hrnet_forward": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                     _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_encoder_forward": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_fuse_forward": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                    _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_decoder_forward": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_void_p, _c.c_void_p]),
    "hrn_hrnet_train_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "hrn_hrnet_forward_train": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward": (_c.c_int, [_c.c_void_p, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                      _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_forward_train_dt": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward_dt": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                         _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_packed_bytes_s": (_c.c_size_t, [_c.c_int] * 3),
    "hrn_hrnet_pack_s": (_c.c_int, [_c.POINTER(HrnetParams), _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_forward_s": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                       _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_decoder_forward_s": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_void_p, _c.c_void_p]),
    "hrn_hrnet_forward_train_s": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                             _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward_s": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams), _c.c_void_p,
                                        _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward_in": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p,
                                         _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams), _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward_sel": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p,
                                          _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams), _c.c_void_p,
                                          _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_masked_composite": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 5 + [_c.c_void_p] * 4),
    "hrn_upsample": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int64] + [_c.c_int] * 3 + [_c.c_float, _c.c_void_p]),
    "hrn_upsample_backward": (_c.c_int, [_c.c_void_p] * 2 + [_c.c_int64] + [_c.c_int] * 3 + [_c.c_float, _c.c_void_p]),
    "hrn_shift_add": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 5 + [_c.c_float, _c.c_float, _c.c_void_p]),
    "hrn_shift_add_backward": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 5 + [_c.c_float, _c.c_float, _c.c_void_p]),
    "hrn_observe_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_observe": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 5 + [_c.c_void_p]),
    "hrn_consistency_residual": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_size_t] + [_c.c_int] * 5 + [_c.c_void_p]),
    "hrn_consistency_finish": (_c.c_int, [_c.c_void_p, _c.c_size_t] + [_c.c_void_p] * 7 + [_c.c_int] * 5 + [_c.c_float, _c.c_int, _c.c_void_p]),
    "hrn_observe_adjoint": (_c.c_int, [_c.c_void_p] * 9 + [_c.c_int] * 5 + [_c.c_void_p]),
    "hrn_observe_shift_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_observe_shift_grad": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_size_t] + [_c.c_int] * 5 + [_c.c_void_p]),
    "hrn_observe_shift_grad_finish": (_c.c_int, [_c.c_void_p, _c.c_size_t] + [_c.c_void_p] * 3 + [_c.c_int] * 4 + [_c.c_void_p]),
    "hrn_shift_normal": (_c.c_int, [_c.c_void_p] * 6 + [_c.c_float] + [_c.c_void_p] * 2 + [_c.c_size_t, _c.c_void_p, _c.c_size_t] + [_c.c_int] * 5
                         + [_c.c_void_p]),
    "hrn_shift_normal_finish": (_c.c_int, [_c.c_void_p, _c.c_size_t] + [_c.c_void_p] * 5 + [_c.c_int] * 6 + [_c.c_float] * 2 + [_c.c_void_p]),
    "hrn_robust_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_robust_sums": (_c.c_int, [_c.c_void_p] * 6 + [_c.c_size_t] + [_c.c_int] * 5 + [_c.c_float, _c.c_void_p]),
    "hrn_robust_finish": (_c.c_int, [_c.c_void_p, _c.c_size_t] + [_c.c_void_p] * 4 + [_c.c_int] * 5 + [_c.c_void_p]),
    "hrn_robust_apply": (_c.c_int, [_c.c_void_p] * 7 + [_c.c_int] * 5 + [_c.c_float, _c.c_void_p]),
    "hrn_btv_step": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 4 + [_c.c_float, _c.c_float, _c.c_void_p]),
    "hrn_btv_backward": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 4 + [_c.c_float, _c.c_float, _c.c_void_p]),
    "hrn_btv_workspace_bytes": (_c.c_size_t, [_c.c_int] * 3),
    "hrn_btv_value": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_size_t] + [_c.c_int] * 4 + [_c.c_float] * 3 + [_c.c_void_p]),
    "hrn_hrnet_forward_ref": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_forward_train_ref": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_hrnet_backward_ref": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(HrnetParams), _c.c_int, _c.c_void_p, _c.c_void_p,
                                          _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(HrnetParams),
                                          _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_packed_bytes": (_c.c_size_t, []),
    "hrn_shiftnet_pack": (_c.c_int, [_c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_workspace_bytes": (_c.c_size_t, [_c.c_int]),
    "hrn_shiftnet_forward": (_c.c_int, [_c.c_void_p, _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_int, _c.c_int, _c.c_float,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_train_workspace_bytes": (_c.c_size_t, [_c.c_int]),
    "hrn_shiftnet_forward_train": (_c.c_int, [_c.c_void_p, _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_int, _c.c_float, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_backward": (_c.c_int, [_c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                         _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_train_workspace_bytes_dt": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "hrn_shiftnet_forward_train_dt": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_int, _c.c_float,
                                                 _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_backward_dt": (_c.c_int, [_c.POINTER(ShiftnetParams), _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                            _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shiftnet_backward_sel": (_c.c_int, [_c.POINTER(ShiftnetParams), _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                             _c.POINTER(ShiftnetParams), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_adam_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_float, _c.c_float, _c.c_float,
                                 _c.c_float, _c.c_float, _c.c_int, _c.c_void_p]),
    "hrn_grad_sumsq_workspace_bytes": (_c.c_size_t, [_c.c_size_t]),
    "hrn_grad_sumsq": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_optim_prepare": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_void_p,
                                     _c.c_void_p]),
    "hrn_adam_step_ex": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_size_t] + [_c.c_float] * 4 + [_c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p]),
    "hrn_lanczos_kernel": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_lanczos_shift": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_lanczos_shift_backward_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_lanczos_shift_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_get_loss": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_get_loss_train_workspace_bytes": (_c.c_size_t, [_c.c_int]),
    "hrn_get_loss_train": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                      _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_get_loss_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_shift_cpsnr_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "hrn_shift_cpsnr": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                   _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_shift_loss_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_shift_loss_train": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p] + [_c.c_int] * 6 + [_c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                                                                  _c.c_size_t, _c.c_void_p]),
    "hrn_shift_loss_backward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 6 + [_c.c_void_p, _c.c_void_p]),
    "hrn_shift_cssim_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "hrn_shift_cssim": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 7 + [_c.c_float] + [_c.c_void_p] * 4 + [_c.c_size_t, _c.c_void_p]),
    "hrn_cssim_loss_backward_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "hrn_cssim_loss_backward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 7 + [_c.c_float] + [_c.c_void_p] * 2 + [_c.c_size_t, _c.c_void_p]),
    "hrn_cl1_loss_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_cl1_loss_train": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 5 + [_c.c_float] + [_c.c_void_p] * 3 + [_c.c_size_t, _c.c_void_p]),
    "hrn_cl1_loss_backward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 5 + [_c.c_float] + [_c.c_void_p] * 2),
    "hrn_mncc_grid": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 5 + [_c.c_float, _c.c_void_p, _c.c_void_p]),
    "hrn_mncc_search": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_mncc_apply": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 4 + [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_mncc_scene_workspace_bytes": (_c.c_size_t, [_c.c_int] * 5),
    "hrn_mncc_grid_scene": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 5 + [_c.c_float, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "hrn_mncc_search_scene": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 6 + [_c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                                             _c.c_void_p]),
    "hrn_mncc_apply_scene": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 4 + [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_mncc_apply_backward_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_mncc_apply_backward": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 4 + [_c.c_void_p] * 3 + [_c.c_size_t, _c.c_void_p]),
    "hrn_subpixel_loss_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "hrn_subpixel_loss_train": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 6 + [_c.c_float, _c.c_int] + [_c.c_void_p] * 4
                                + [_c.c_size_t, _c.c_void_p]),
    "hrn_subpixel_loss_backward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 5 + [_c.c_void_p] * 2 + [_c.c_size_t, _c.c_void_p]),
    "hrn_mncc_local_blocks": (_c.c_int, [_c.c_int] * 2),
    "hrn_mncc_local_workspace_bytes": (_c.c_size_t, [_c.c_int] * 6),
    "hrn_mncc_search_local": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 6 + [_c.c_float, _c.c_int, _c.c_float] + [_c.c_void_p] * 4
                              + [_c.c_size_t, _c.c_void_p]),
    "hrn_mncc_apply_field": (_c.c_int, [_c.c_void_p] * 3 + [_c.c_int] * 5 + [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_mncc_reduce2": (_c.c_int, [_c.c_void_p] * 2 + [_c.c_int] * 3 + [_c.c_void_p] * 3),
    "hrn_mncc_search_scene_from": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int] * 6 + [_c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                                                  _c.c_void_p]),
    "hrn_mncc_pyramid_workspace_bytes": (_c.c_size_t, [_c.c_int] * 6),
    "hrn_mncc_search_pyramid": (_c.c_int, [_c.c_void_p] * 4 + [_c.c_int] * 7 + [_c.c_float, _c.c_int, _c.c_float] + [_c.c_void_p] * 3
                                + [_c.c_size_t, _c.c_void_p]),
    "hrn_collate_device": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                      _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_collate_device_s": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p]),
    "hrn_collate_device_a": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p]),
    "hrn_collate_device_m": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                        _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_dihedral_expand": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_dihedral_mean": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int32), _c.c_int, _c.c_void_p, _c.c_void_p]),
    "hrn_hrnet_halo": (_c.c_int, [_c.c_int, _c.c_int]),
    "hrn_tile_count": (_c.c_int, [_c.c_int] * 4),
    "hrn_tile_gather": (_c.c_int, [_c.c_void_p] + [_c.c_int] * 8 + [_c.c_void_p, _c.c_void_p]),
    "hrn_tile_scatter": (_c.c_int, [_c.c_void_p] + [_c.c_int] * 8 + [_c.c_void_p, _c.c_void_p]),
    "hrn_resample_targets": (_c.c_int, [_c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "hrn_profile_enable": (_c.c_int, [_c.c_int]),
    "hrn_profile_count": (_c.c_int, []),
    "hrn_profile_get": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int, _c.POINTER(_c.c_long), _c.POINTER(_c.c_double),
                                   _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
}

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen the in-tree library and type every entry point.  Raises if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python highres-net_amd/hrnet_hip/build.py` "
                "(or __graft_entry__.build()).  There is no CPU / PyTorch fallback for the HIP path.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError here == ABI mismatch: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


class HrnetHipError(RuntimeError):
    pass


def has_bf16x3():
    """True when the loaded library implements the split-bf16 precision mode (HRN_DTYPE_BF16X3)."""
    return load_library().hrn_hrnet_packed_bytes(BF16X3, 2) != 0


def _check(rc, what):
    if rc != 0:
        msg = load_library().hrn_last_error().decode("utf-8", "replace")
        raise HrnetHipError(f"{what} failed with code {rc}: {msg}")


def _dev_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on '{t.device}': the HIP path needs ROCm device tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------- HRNet
def hrnet_param_table(num_layers):
    """HRNet's parameters in the module's registration order (== the reference's state_dict order, HRNet.py:36-169), one row each:
    (state-dict key, HrnetParams field, index into that field's array or None)."""
    def block(prefix, field, first):          # a ResidualBlock: conv, PReLU, conv, PReLU
        return [(f"{prefix}.block.{m}.{leaf}", f"{field}_{x}", first + j)
                for j in (0, 1) for m, leaf, x in ((2 * j, "weight", "w"), (2 * j, "bias", "b"), (2 * j + 1, "weight", "a"))]

    rows = [("encode.init_layer.0.weight", "enc_init_w", None), ("encode.init_layer.0.bias", "enc_init_b", None),
            ("encode.init_layer.1.weight", "enc_init_a", None)]
    for l in range(num_layers):
        rows += block(f"encode.res_layers.{l}", "enc_res", 2 * l)
    rows += [("encode.final.0.weight", "enc_final_w", None), ("encode.final.0.bias", "enc_final_b", None)]
    rows += block("fuse.fuse.0", "fuse_res", 0)
    rows += [("fuse.fuse.1.weight", "fuse_out_w", None), ("fuse.fuse.1.bias", "fuse_out_b", None), ("fuse.fuse.2.weight", "fuse_out_a", None),
             ("decode.deconv.0.weight", "dec_w", None), ("decode.deconv.0.bias", "dec_b", None), ("decode.deconv.1.weight", "dec_a", None),
             ("decode.final.weight", "fin_w", None), ("decode.final.bias", "fin_b", None)]
    return rows


def hrnet_param_names(num_layers):
    """HRNet's parameters in the module's registration order (== the reference's state_dict order, HRNet.py:36-169)."""
    return [key for key, _, _ in hrnet_param_table(num_layers)]


def hrnet_param_struct(named, num_layers, optional=False):
    """named: dict of reference state-dict keys -> device f32 tensors.  Returns (HrnetParams, tensors kept alive).  optional: a key
    missing from `named` becomes a NULL field (a frozen parameter's gradient for hrn_hrnet_backward_sel)."""
    keep = []
    P = HrnetParams()
    P.num_layers = num_layers
    for key, field, index in hrnet_param_table(num_layers):
        if optional and key not in named:
            continue                          # (a fresh struct is all NULL)
        t = _dev_f32(named[key].detach(), key)
        keep.append(t)
        if index is None:
            setattr(P, field, t.data_ptr())
        else:
            getattr(P, field)[index] = t.data_ptr()
    return P, keep


SCALES = (2, 3, 4)       # upscale factors the decoder kernels are built for (deconv kernel_size == stride)


def hrnet_pack(named, num_layers, dtype, scale=3):
    """named: dict of reference state-dict keys -> device f32 tensors (decode.deconv.0.weight (64,64,scale,scale)).  Returns the
    packed uint8 tensor, valid for this dtype and scale only."""
    lib = load_library()
    nbytes = lib.hrn_hrnet_packed_bytes_s(dtype, num_layers, scale)
    if nbytes == 0:
        raise HrnetHipError(f"unsupported dtype/num_layers/scale ({dtype}, {num_layers}, {scale})")
    w = named["decode.deconv.0.weight"]
    if tuple(w.shape) != (64, 64, scale, scale):
        raise ValueError(f"decode.deconv.0.weight is {tuple(w.shape)}; scale {scale} needs (64, 64, {scale}, {scale})")
    P, keep = hrnet_param_struct(named, num_layers)
    dev = keep[0].device
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.hrn_hrnet_pack_s(ctypes.byref(P), dtype, scale, _ptr(packed), nbytes, _stream()), "hrn_hrnet_pack")
    return packed


_ws_cache = {}


def _workspace(nbytes, device, tag):
    key = (tag, device.index)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _ws_cache.pop(key, None)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def hrnet_workspace(dtype, B, V, H, W, device):
    n = load_library().hrn_hrnet_workspace_bytes(dtype, B, V, H, W)
    if n == 0:
        raise HrnetHipError(f"bad HRNet problem size B={B} V={V} H={H} W={W}")
    return _workspace(n, device, "hrnet")


def _ref_frame(ref, lrs):
    """the reference frame given to the network: a float (B,H,W) tensor on the device of lrs (B,V,H,W) -> contiguous f32"""
    if not isinstance(ref, torch.Tensor):
        raise TypeError(f"ref must be a torch.Tensor, got {type(ref).__name__}")
    if not ref.is_floating_point():
        raise TypeError(f"ref must be a floating-point tensor, got {ref.dtype}")
    want = (lrs.shape[0],) + tuple(lrs.shape[2:])
    if tuple(ref.shape) != want:
        raise ValueError(f"ref must be (B,H,W) = {want} for lrs {tuple(lrs.shape)}; got {tuple(ref.shape)}")
    if ref.device != lrs.device:
        raise RuntimeError(f"ref is on '{ref.device}' but lrs on '{lrs.device}': the reference frame must be on the views' device")
    return ref.float().contiguous()


def hrnet_forward(packed, dtype, num_layers, alpha_residual, lrs, alphas, out=None, scale=3, ref=None):
    """-> sr (B, 1, scale H, scale W); `packed` is the blob of hrnet_pack at this dtype and scale.  ref (B,H,W): the reference frame in place
    of the median of lrs[:, :9] (hrn_hrnet_forward_ref)."""
    lib = load_library()
    lrs = _dev_f32(lrs, "lrs")
    alphas = _dev_f32(alphas, "alphas").to(lrs.device)
    if lrs.dim() != 4 or alphas.shape != lrs.shape[:2]:
        raise ValueError(f"lrs must be (B,V,H,W) and alphas (B,V); got {tuple(lrs.shape)} / {tuple(alphas.shape)}")
    B, V, H, W = lrs.shape
    if ref is not None:
        ref = _ref_frame(ref, lrs)
    with torch.cuda.device(lrs.device):
        ws = hrnet_workspace(dtype, B, V, H, W, lrs.device)
        if out is not None and (tuple(out.shape) != (B, 1, scale * H, scale * W) or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(B, 1, scale * H, scale * W)}")
        sr = out if out is not None else torch.empty((B, 1, scale * H, scale * W), dtype=torch.float32, device=lrs.device)
        if ref is not None:
            _check(lib.hrn_hrnet_forward_ref(_ptr(packed), dtype, num_layers, scale, int(bool(alpha_residual)), _ptr(lrs), _ptr(alphas),
                                             _ptr(ref), B, V, H, W, _ptr(sr), _ptr(ws), ws.numel(), _stream()), "hrn_hrnet_forward_ref")
            return sr
        _check(lib.hrn_hrnet_forward_s(_ptr(packed), dtype, num_layers, scale, int(bool(alpha_residual)), _ptr(lrs), _ptr(alphas),
                                       B, V, H, W, _ptr(sr), _ptr(ws), ws.numel(), _stream()), "hrn_hrnet_forward")
    return sr


def hrnet_encoder(packed, dtype, num_layers, lrs):
    """-> view stack (B,V,H,W,64) channels-last in the storage dtype ((2,B,V,H,W,64) bf16 planes for BF16X3)."""
    lib = load_library()
    lrs = _dev_f32(lrs, "lrs")
    B, V, H, W = lrs.shape
    with torch.cuda.device(lrs.device):
        ws = hrnet_workspace(dtype, B, V, H, W, lrs.device)
        emb = torch.empty(((2,) if dtype == BF16X3 else ()) + (B, V, H, W, 64), dtype=_DT_TORCH[dtype], device=lrs.device)
        _check(lib.hrn_encoder_forward(_ptr(packed), dtype, num_layers, _ptr(lrs), B, V, H, W, _ptr(emb), _ptr(ws), ws.numel(),
                                       _stream()), "hrn_encoder_forward")
    return emb


def hrnet_fuse(packed, dtype, num_layers, alpha_residual, emb, alphas):
    """emb (B,V,H,W,64) storage dtype (destroyed) -> fused (B,H,W,64); BF16X3: both with a leading plane axis of 2."""
    lib = load_library()
    if emb.dtype != _DT_TORCH[dtype] or not emb.is_contiguous() or not emb.is_cuda or emb.dim() != (6 if dtype == BF16X3 else 5):
        raise ValueError("emb must be a contiguous device tensor in the storage dtype")
    B, V, H, W, _ = emb.shape[-5:]
    alphas = _dev_f32(alphas, "alphas")
    with torch.cuda.device(emb.device):
        ws = hrnet_workspace(dtype, B, V, H, W, emb.device)
        fused = torch.empty(((2,) if dtype == BF16X3 else ()) + (B, H, W, 64), dtype=emb.dtype, device=emb.device)
        _check(lib.hrn_fuse_forward(_ptr(packed), dtype, num_layers, int(bool(alpha_residual)), _ptr(emb), _ptr(alphas),
                                    B, V, H, W, _ptr(fused), _ptr(ws), ws.numel(), _stream()), "hrn_fuse_forward")
    return fused


def hrnet_decoder(packed, dtype, num_layers, fused, scale=3):
    """fused (N,H,W,64) in the storage dtype ((2,N,H,W,64) planes for BF16X3) -> sr (N, 1, scale H, scale W)."""
    lib = load_library()
    if fused.dtype != _DT_TORCH[dtype] or not fused.is_contiguous() or not fused.is_cuda or fused.dim() != (5 if dtype == BF16X3 else 4):
        raise ValueError("fused must be a contiguous device tensor in the storage dtype")
    N, H, W, _ = fused.shape[-4:]
    with torch.cuda.device(fused.device):
        sr = torch.empty((N, 1, scale * H, scale * W), dtype=torch.float32, device=fused.device)
        _check(lib.hrn_decoder_forward_s(_ptr(packed), dtype, num_layers, scale, _ptr(fused), N, H, W, _ptr(sr), _stream()),
               "hrn_decoder_forward")
    return sr


def hrnet_forward_train(packed_f32, lrs, alphas, num_layers, alpha_residual, dtype=F32, scale=3, ref=None):
    """Training forward: returns (sr, train_ws); train_ws holds every intermediate for hrnet_backward.  dtype F32 (exact-fp32 MFMA),
    BF16X3 (split-bf16: `packed_f32` is then the BF16X3 blob and the workspace holds pairs of bf16 planes) or BF16 (`packed_f32` the BF16
    blob, one bf16 plane per activation, fp32 accumulation).  ref (B,H,W) contiguous f32: the reference frame in place of the median
    (hrn_hrnet_forward_train_ref); it is read in place, so hand the same, unchanged tensor to hrnet_backward."""
    lib = load_library()
    lrs = _dev_f32(lrs, "lrs")
    alphas = _dev_f32(alphas, "alphas")
    B, V, H, W = lrs.shape
    if ref is not None:
        ref = _ref_frame(ref, lrs)
    nbytes = lib.hrn_hrnet_train_workspace_bytes(num_layers, B, V, H, W)
    if nbytes == 0:
        raise HrnetHipError(f"bad training shape B={B} V={V} H={H} W={W} num_layers={num_layers}")
    tws = torch.empty(nbytes, dtype=torch.uint8, device=lrs.device)
    sr = torch.empty((B, 1, scale * H, scale * W), dtype=torch.float32, device=lrs.device)
    with torch.cuda.device(lrs.device):
        if ref is not None:
            _check(lib.hrn_hrnet_forward_train_ref(_ptr(packed_f32), int(dtype), num_layers, int(scale), int(bool(alpha_residual)), _ptr(lrs),
                                                   _ptr(alphas), _ptr(ref), B, V, H, W, _ptr(sr), _ptr(tws), nbytes, _stream()),
                   "hrn_hrnet_forward_train_ref")
            return sr, tws
        _check(lib.hrn_hrnet_forward_train_s(_ptr(packed_f32), int(dtype), num_layers, int(scale), int(bool(alpha_residual)), _ptr(lrs),
                                             _ptr(alphas), B, V, H, W, _ptr(sr), _ptr(tws), nbytes, _stream()), "hrn_hrnet_forward_train")
    return sr, tws


def hrnet_backward(packed_f32, named_params, named_grads, num_layers, alpha_residual, lrs, alphas, d_sr, tws, dtype=F32, scale=3,
                   d_lrs=None, d_alphas=None, select=False, ref=None, d_ref=None):
    """Accumulates dLoss/dparam into named_grads (same keys / shapes as named_params, f32, zero them for plain gradients).  d_lrs
    (B,V,H,W) / d_alphas (B,V): contiguous f32 device tensors that receive (are overwritten with) the input gradients, or None.
    select: named_grads holds only the parameters that want a gradient (the work of the others is skipped); otherwise it must hold
    every parameter.  One C call either way: hrn_hrnet_backward_sel, which leaves out whatever a NULL field or pointer does not ask for.
    ref (B,H,W): the reference frame the training forward was given (hrn_hrnet_backward_ref); d_lrs is then the stem's channel 0 alone, and
    d_ref (B,H,W) or None receives the frame's gradient."""
    lib = load_library()
    lrs = _dev_f32(lrs, "lrs")
    alphas = _dev_f32(alphas, "alphas")
    d_sr = _dev_f32(d_sr, "d_sr")
    B, V, H, W = lrs.shape
    if tuple(d_sr.shape) != (B, 1, scale * H, scale * W):
        raise ValueError(f"d_sr shape {tuple(d_sr.shape)} != {(B, 1, scale * H, scale * W)}")
    P, keep_p = hrnet_param_struct(named_params, num_layers)
    G, keep_g = hrnet_param_struct(named_grads, num_layers, optional=select)
    pairs = zip(keep_p, keep_g) if not select else ((named_params[k], g) for k, g in named_grads.items())
    for t, g in pairs:
        if t.shape != g.shape or g.data_ptr() == t.data_ptr():
            raise ValueError("gradient buffers must match the parameters' shapes and not alias them")
    if select and (set(named_grads) - set(hrnet_param_names(num_layers))):
        raise ValueError(f"unknown HRNet parameters among the gradients: {sorted(set(named_grads) - set(hrnet_param_names(num_layers)))}")
    if ref is not None:
        ref = _ref_frame(ref, lrs)
    elif d_ref is not None:
        raise ValueError("d_ref needs ref: without an outside frame its gradient is routed into d_lrs")
    for name, t, shape in (("d_lrs", d_lrs, (B, V, H, W)), ("d_alphas", d_alphas, (B, V)), ("d_ref", d_ref, (B, H, W))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != lrs.device):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {lrs.device}")
    opt = lambda t: _ptr(t) if t is not None else None
    with torch.cuda.device(lrs.device):
        if ref is not None:
            _check(lib.hrn_hrnet_backward_ref(_ptr(packed_f32), int(dtype), int(scale), ctypes.byref(P), int(bool(alpha_residual)),
                                              _ptr(lrs), _ptr(alphas), _ptr(ref), B, V, H, W, _ptr(d_sr), ctypes.byref(G), opt(d_lrs),
                                              opt(d_alphas), opt(d_ref), _ptr(tws), tws.numel(), _stream()), "hrn_hrnet_backward_ref")
            return
        _check(lib.hrn_hrnet_backward_sel(_ptr(packed_f32), int(dtype), int(scale), ctypes.byref(P), int(bool(alpha_residual)),
                                          _ptr(lrs), _ptr(alphas), B, V, H, W, _ptr(d_sr), ctypes.byref(G),
                                          _ptr(d_lrs) if d_lrs is not None else None, _ptr(d_alphas) if d_alphas is not None else None,
                                          _ptr(tws), tws.numel(), _stream()), "hrn_hrnet_backward")


# --------------------------------------------------------------------------- ShiftNet
def _shiftnet_struct(named, keep, with_weights, optional=False):
    P = ShiftnetParams()

    def p(key):
        if optional and key not in named:
            return None                                      # a frozen parameter's gradient (hrn_shiftnet_backward_sel)
        t = named[key].detach()
        if not t.is_cuda:
            raise RuntimeError(f"{key} is on '{t.device}': ShiftNet parameters must live on the ROCm device")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{key} must be contiguous float32")
        keep.append(t)
        return t.data_ptr()

    for i in range(8):
        if with_weights:
            P.conv_w[i], P.conv_b[i] = p(f"layer{i + 1}.0.weight"), p(f"layer{i + 1}.0.bias")
        P.bn_g[i], P.bn_b[i] = p(f"layer{i + 1}.1.weight"), p(f"layer{i + 1}.1.bias")
        P.bn_rm[i], P.bn_rv[i] = p(f"layer{i + 1}.1.running_mean"), p(f"layer{i + 1}.1.running_var")
    if with_weights:
        P.fc1_w, P.fc1_b, P.fc2_w = p("fc1.weight"), p("fc1.bias"), p("fc2.weight")
    return P


def shiftnet_pack(named):
    lib = load_library()
    keep = []
    P = _shiftnet_struct(named, keep, True)
    dev = keep[0].device
    nbytes = lib.hrn_shiftnet_packed_bytes()
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.hrn_shiftnet_pack(ctypes.byref(P), _ptr(packed), nbytes, _stream()), "hrn_shiftnet_pack")
    return packed


def _check_shiftnet_input(x, dropout_mask):
    if x.dim() != 4 or tuple(x.shape[1:]) != (2, 128, 128):
        raise ValueError(f"ShiftNet input must be (B,2,128,128) (fc1 is hard-wired to 128*16*16, ShiftNet.py:44); got {tuple(x.shape)}")
    B = x.shape[0]
    if dropout_mask is None:
        return ctypes.c_void_p(0), None
    if dropout_mask.dtype != torch.uint8 or tuple(dropout_mask.shape) != (B, 32768) or not dropout_mask.is_cuda:
        raise ValueError("dropout_mask must be a uint8 device tensor of shape (B, 32768)")
    dropout_mask = dropout_mask.contiguous()
    return _ptr(dropout_mask), dropout_mask


def shiftnet_forward(packed, named, x, train_bn=False, momentum=0.1, dropout_mask=None):
    """x (B,2,128,128) -> theta (B,2).  `named` supplies the live BatchNorm tensors (running stats are updated in
    place when train_bn) and fc1.weight, which the kernel reads in place.  dropout_mask: None or uint8 (B,32768) keep-mask in the reference's flatten order."""
    lib = load_library()
    x = _dev_f32(x, "x")
    mptr, dropout_mask = _check_shiftnet_input(x, dropout_mask)
    B = x.shape[0]
    keep = []
    P = _shiftnet_struct(named, keep, True)        # (fc1.weight is read in place by the kernel: not part of `packed`)
    with torch.cuda.device(x.device):
        nws = lib.hrn_shiftnet_workspace_bytes(B)
        ws = _workspace(nws, x.device, "shiftnet")
        theta = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        _check(lib.hrn_shiftnet_forward(_ptr(packed), ctypes.byref(P), _ptr(x), B, int(bool(train_bn)), float(momentum), mptr,
                                        _ptr(theta), _ptr(ws), ws.numel(), _stream()), "hrn_shiftnet_forward")
    return theta


def shiftnet_forward_train(packed, named, x, momentum=0.1, dropout_mask=None, dtype=F32):
    """Train-mode forward that keeps its intermediates: returns (theta (B,2), train_ws).  dtype: storage of the workspace's activations,
    F32 or BF16; `packed` is the fp32 blob in both."""
    lib = load_library()
    x = _dev_f32(x, "x")
    mptr, dropout_mask = _check_shiftnet_input(x, dropout_mask)
    B = x.shape[0]
    keep = []
    P = _shiftnet_struct(named, keep, True)        # (fc1.weight is read in place by the kernel: not part of `packed`)
    nbytes = lib.hrn_shiftnet_train_workspace_bytes_dt(int(dtype), B)
    if nbytes == 0:
        raise ValueError(f"ShiftNet training supports dtype F32 ({F32}) or BF16 ({BF16}); got {dtype}")
    tws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    theta = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.hrn_shiftnet_forward_train_dt(_ptr(packed), int(dtype), ctypes.byref(P), _ptr(x), B, float(momentum), mptr,
                                                 _ptr(theta), _ptr(tws), nbytes, _stream()), "hrn_shiftnet_forward_train")
    return theta, tws


def shiftnet_backward(named, named_grads, x, dropout_mask, d_theta, tws, need_input_grad=True, dtype=F32, select=False):
    """Accumulates the parameter gradients into named_grads (parameter keys only); returns d_x (B,2,128,128) or None.  dtype: the
    forward's (the workspace `tws` it filled).  select: named_grads holds only the parameters that want a gradient (the work of the
    others is skipped).  One C call either way: hrn_shiftnet_backward_sel."""
    lib = load_library()
    x = _dev_f32(x, "x")
    d_theta = _dev_f32(d_theta, "d_theta")
    mptr, dropout_mask = _check_shiftnet_input(x, dropout_mask)
    B = x.shape[0]
    keep = []
    P = _shiftnet_struct(named, keep, True)
    gfull = dict(named_grads)
    for k, v in named.items():                               # the struct builder also wants the (unused) running stats
        if not select or k in SHIFTNET_BUFFER_NAMES:
            gfull.setdefault(k, v)
    G = _shiftnet_struct(gfull, keep, True, optional=select)
    d_x = torch.empty_like(x) if need_input_grad else None
    with torch.cuda.device(x.device):
        _check(lib.hrn_shiftnet_backward_sel(ctypes.byref(P), int(dtype), _ptr(x), B, mptr, _ptr(d_theta), ctypes.byref(G),
                                             _ptr(d_x) if need_input_grad else None, _ptr(tws), tws.numel(), _stream()),
               "hrn_shiftnet_backward")
    return d_x


# --------------------------------------------------------------------------- Lanczos
def lanczos_kernel(dx):
    lib = load_library()
    dx = _dev_f32(dx, "dx").reshape(-1)
    n = dx.numel()
    taps = torch.empty((n, 7), dtype=torch.float32, device=dx.device)
    with torch.cuda.device(dx.device):
        _check(lib.hrn_lanczos_kernel(_ptr(dx), n, _ptr(taps), _stream()), "hrn_lanczos_kernel")
    return taps


def lanczos_shift(img, shift):
    lib = load_library()
    img = _dev_f32(img, "img")
    shift = _dev_f32(shift, "shift").to(img.device)
    if img.dim() != 4 or shift.dim() != 2 or shift.shape[1] != 2 or shift.shape[0] < img.shape[1]:
        raise ValueError(f"img must be (b,c,H,W) and shift (c,2); got {tuple(img.shape)} / {tuple(shift.shape)}")
    b, c, H, W = img.shape
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _check(lib.hrn_lanczos_shift(_ptr(img), _ptr(shift), b, c, H, W, _ptr(out), _stream()), "hrn_lanczos_shift")
    return out


def lanczos_shift_backward(img, shift, d_out, need_img=True, need_shift=True):
    """Gradients of lanczos_shift(img, shift) given d_out: (d_img or None, d_shift (c, 2) or None)."""
    lib = load_library()
    img, shift, d_out = _dev_f32(img, "img"), _dev_f32(shift, "shift"), _dev_f32(d_out, "d_out")
    b, c, H, W = img.shape
    nbytes = lib.hrn_lanczos_shift_backward_workspace_bytes(b, c, H, W)
    ws = _workspace(nbytes, img.device, "lanczos_bwd")
    d_img = torch.empty_like(img) if need_img else None
    d_shift = torch.zeros((c, 2), dtype=torch.float32, device=img.device) if need_shift else None
    with torch.cuda.device(img.device):
        _check(lib.hrn_lanczos_shift_backward(_ptr(img), _ptr(shift), _ptr(d_out), b, c, H, W,
                                              _ptr(d_img) if need_img else None, _ptr(d_shift) if need_shift else None,
                                              _ptr(ws), ws.numel(), _stream()), "hrn_lanczos_shift_backward")
    return d_img, d_shift


# --------------------------------------------------------------------------- optimiser
# Bumped by anything that rewrites parameter storage without going through torch's version counters (the fused Adam
# kernel writes the flat buffer the parameters are views of); the modules' packed-parameter caches key on it.
param_epoch = 0


def bump_param_epoch():
    global param_epoch
    param_epoch += 1


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step):
    """In-place Adam update of the flat fp32 device buffer `params` (torch.optim.Adam arithmetic, no amsgrad)."""
    lib = load_library()
    for name, t in (("params", params), ("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == params.numel()):
            raise ValueError(f"{name} must be a contiguous float32 device tensor of {params.numel()} elements")
    with torch.cuda.device(params.device):
        _check(lib.hrn_adam_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), float(lr), float(beta1),
                                 float(beta2), float(eps), float(weight_decay), int(step), _stream()), "hrn_adam_step")
    bump_param_epoch()


# The guarded step (csrc/optim_guard.hip).  One step-control block per parameter group, as include/hrnet_hip.h lays hrn_optim_ctl out;
# a (G, OPTIM_CTL_WORDS) int64 device tensor holds G of them.
OPTIM_MAX_GROUPS = 8
OPTIM_CTL_BYTES = 48
OPTIM_CTL_WORDS = OPTIM_CTL_BYTES // 8
OPTIM_CTL_FIELDS = {"applied": (0, torch.int64), "skipped": (8, torch.int64), "norm": (16, torch.float64), "coef": (24, torch.float32),
                    "step_size": (28, torch.float32), "inv_bc2_sqrt": (32, torch.float32), "lr": (36, torch.float32),
                    "skip": (40, torch.int32)}


def optim_ctl_field(ctl, group, name):
    """A 0-d view of one field of the control block of `group` in `ctl` (a (G, OPTIM_CTL_WORDS) int64 device tensor); no sync."""
    off, dtype = OPTIM_CTL_FIELDS[name]
    row = ctl[group].view(torch.uint8)
    return row[off:off + torch.empty((), dtype=dtype).element_size()].view(dtype)[0]


def _flat_f32(name, t, n=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and (n is None or t.numel() == n)):
        raise ValueError(f"{name} must be a contiguous 1-d float32 device tensor" + (f" of {n} elements" if n is not None else ""))


def _optim_ctl(ctl, n_groups):
    if not (ctl.is_cuda and ctl.dtype == torch.int64 and ctl.is_contiguous() and tuple(ctl.shape) == (n_groups, OPTIM_CTL_WORDS)):
        raise ValueError(f"ctl must be a contiguous int64 device tensor of shape ({n_groups}, {OPTIM_CTL_WORDS})")


def grad_sumsq(grads):
    """(sum of g^2 over the finite elements, number of non-finite elements) of a flat fp32 device buffer, as a float64 (2,) device
    tensor: fp64 accumulation in a fixed order, bit-reproducible, no sync."""
    lib = load_library()
    _flat_f32("grads", grads)
    n = grads.numel()
    out = torch.empty(2, dtype=torch.float64, device=grads.device)
    nbytes = lib.hrn_grad_sumsq_workspace_bytes(n)
    ws = _workspace(nbytes, grads.device, "grad_sumsq")
    with torch.cuda.device(grads.device):
        _check(lib.hrn_grad_sumsq(_ptr(grads), n, _ptr(out), _ptr(ws), ws.numel(), _stream()), "hrn_grad_sumsq")
    return out


def optim_prepare(sums, ctl, group, max_norm, lr, beta1, beta2):
    """sums: (G, 2) float64, every group's grad_sumsq.  Updates the control block ctl[group] in place (norm, coef, skip, the counters
    and the bias corrections of the group whose lr / betas are given).  max_norm <= 0: no clipping."""
    lib = load_library()
    if not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and sums.dim() == 2 and sums.shape[1] == 2):
        raise ValueError("sums must be a contiguous float64 device tensor of shape (n_groups, 2)")
    G = sums.shape[0]
    if not 1 <= G <= OPTIM_MAX_GROUPS:
        raise ValueError(f"n_groups must be in 1..{OPTIM_MAX_GROUPS} (got {G})")
    _optim_ctl(ctl, G)
    with torch.cuda.device(sums.device):
        _check(lib.hrn_optim_prepare(_ptr(sums), G, int(group), float(max_norm), float(lr), float(beta1), float(beta2), _ptr(ctl),
                                     _stream()), "hrn_optim_prepare")


def adam_step_ex(params, grads, exp_avg, exp_avg_sq, ema, ctl, group, beta1, beta2, eps, weight_decay, decoupled, ema_decay):
    """The guarded Adam / AdamW update of the flat fp32 buffer `params` under the control block ctl[group]; `ema` (or None) is updated
    towards the new parameters.  `grads` is not written: the clipped gradient exists in registers only."""
    lib = load_library()
    n = params.numel()
    for name, t in (("params", params), ("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("ema", ema)):
        if t is not None:
            _flat_f32(name, t, n)
    if ctl.dim() != 2 or not 0 <= group < ctl.shape[0]:
        raise ValueError(f"group {group} is not a row of ctl")
    _optim_ctl(ctl, ctl.shape[0])
    with torch.cuda.device(params.device):
        _check(lib.hrn_adam_step_ex(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema) if ema is not None else None, n,
                                    float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(decoupled)),
                                    float(ema_decay), ctypes.c_void_p(ctl.data_ptr() + group * OPTIM_CTL_BYTES), _stream()),
               "hrn_adam_step_ex")
    bump_param_epoch()


# --------------------------------------------------------------------------- input pipeline
COLLATE_META = 5          # leading int64 fields of a plan row (HRN_COLLATE_META): hr_off, sm_off, side, row, col


def collate_device(lr_arena, hr_arena, sm_arena, plan, S, lrs, alphas, hrs, maps, scale=3, codes=None, qm_arena=None, lr_masks=None):
    """One launch on the current stream: gather + convert a batch from the device arenas (uint16 LR / HR, uint8 SM) into
    lrs (B,min_L,S,S), alphas (B,min_L), hrs (B,kS,kS) or None, maps (B,kS,kS) f32 with k = `scale` (2, 3 or 4: the HR / LR ratio
    the arenas are stored at), following `plan`, a device int64 (B, COLLATE_META + min_L) table (include/hrnet_hip.h,
    hrn_collate_device_a).  `codes`: None, or a device int32 (B,) tensor of augmentation codes (hrnet_hip/augment.py), one per
    sample; they are not read back, so a code outside 0..7 shows as NaN planes of that sample, not as an error.
    `qm_arena` with `lr_masks` (both or neither): the uint8 arena of LR quality masks, laid out like `lr_arena`, and the
    (B,min_L,S,S) f32 output for the masks of the views in `lrs` - the same launch then writes it too (hrn_collate_device_m)."""
    B, min_L = alphas.shape
    use_hr = hrs is not None
    scale = check_scale(scale)
    if (qm_arena is None) != (lr_masks is None):
        raise ValueError("qm_arena and lr_masks go together: give both or neither")
    arenas = [("lr_arena", lr_arena, torch.uint16), ("sm_arena", sm_arena, torch.uint8), ("plan", plan, torch.int64)]
    if qm_arena is not None:
        arenas.append(("qm_arena", qm_arena, torch.uint8))
    for name, t, dt in arenas + ([("hr_arena", hr_arena, torch.uint16)] if use_hr else []):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.dtype != dt:
            raise RuntimeError(f"{name} must be a contiguous {dt} ROCm device tensor")
    if tuple(plan.shape) != (B, COLLATE_META + min_L):
        raise ValueError(f"plan is {tuple(plan.shape)}, expected {(B, COLLATE_META + min_L)}")
    if codes is not None and not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.is_contiguous() and codes.dtype == torch.int32
                                  and tuple(codes.shape) == (B,)):
        raise ValueError(f"codes must be a contiguous int32 ROCm device tensor of shape {(B,)}")
    outs = [("lrs", lrs, (B, min_L, S, S)), ("alphas", alphas, (B, min_L)), ("maps", maps, (B, scale * S, scale * S))]
    if hrs is not None:
        outs.append(("hrs", hrs, (B, scale * S, scale * S)))
    if lr_masks is not None:
        outs.append(("lr_masks", lr_masks, (B, min_L, S, S)))
    for name, t, shape in outs:
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a contiguous float32 device tensor of shape {shape}")
    head = (_ptr(lr_arena), lr_arena.numel(), _ptr(hr_arena) if use_hr else None, hr_arena.numel() if use_hr else 0, _ptr(sm_arena),
            sm_arena.numel())
    tail = (_ptr(lrs), _ptr(alphas), _ptr(hrs) if use_hr else None, _ptr(maps))
    codes_p = _ptr(codes) if codes is not None else None
    if lr_masks is None:
        _check(load_library().hrn_collate_device_a(*head, _ptr(plan), B, min_L, S, scale, *tail, codes_p, _stream()), "hrn_collate_device_a")
    else:
        _check(load_library().hrn_collate_device_m(*head, _ptr(qm_arena), qm_arena.numel(), _ptr(plan), B, min_L, S, scale, *tail,
                                                   _ptr(lr_masks), codes_p, _stream()), "hrn_collate_device_m")


# --------------------------------------------------------------------------- flip / rotate self-ensemble
def _dihedral_args(t, name, codes, lead):
    """-> (contiguous f32 device tensor, host int32 array of the codes, K, N, H, W); `lead`: leading axes that are not planes."""
    codes = augment.check_codes(codes)
    t = _dev_f32(t, name)
    if t.dim() < 2 + lead:
        raise ValueError(f"{name} must have at least {2 + lead} axes, got {tuple(t.shape)}")
    if lead and t.shape[0] != len(codes):
        raise ValueError(f"{name} has {t.shape[0]} members for {len(codes)} codes")
    H, W = t.shape[-2:]
    N = int(np.prod(t.shape[lead:-2], dtype=np.int64))
    if t.numel() == 0:
        raise ValueError(f"{name} is empty: {tuple(t.shape)}")
    return t, (ctypes.c_int32 * len(codes))(*codes), len(codes), N, H, W


def dihedral_expand(x, codes):
    """x (..., H, W) -> (K, ..., H, W), member-major: out[k] = augment.apply(x, codes[k]).  `codes`: a host sequence of 1..8 distinct
    codes in 0..7 (hrnet_hip/augment.py); one launch of hrn_dihedral_expand on the current stream."""
    x, carr, K, N, H, W = _dihedral_args(x, "x", codes, 0)
    out = torch.empty((K,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(load_library().hrn_dihedral_expand(_ptr(x), N, H, W, carr, K, _ptr(out), _stream()), "hrn_dihedral_expand")
    return out


def dihedral_mean(y, codes):
    """y (K, ..., H, W) -> (..., H, W): the mean over the members of augment.apply(y[k], augment.inverse(codes[k])), summed in fp32
    in list order and multiplied once by float32(1 / K) - bit for bit augment.mean_inverse.  One launch of hrn_dihedral_mean."""
    y, carr, K, N, H, W = _dihedral_args(y, "y", codes, 1)
    out = torch.empty(tuple(y.shape[1:]), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _check(load_library().hrn_dihedral_mean(_ptr(y), N, H, W, carr, K, _ptr(out), _stream()), "hrn_dihedral_mean")
    return out


# --------------------------------------------------------------------------- tiled inference
def hrnet_halo(num_layers, n_views):
    """hrn_hrnet_halo: the network's one-sided receptive field in LR pixels (== tiling.halo)."""
    r = load_library().hrn_hrnet_halo(int(num_layers), int(n_views))
    _check(min(r, 0), "hrn_hrnet_halo")
    return r


def tile_count(H, W, t, R):
    """hrn_tile_count: the number of windows of the plan (== len(tiling.plan(H, W, t, R).windows) for t <= min(H, W))."""
    n = load_library().hrn_tile_count(int(H), int(W), int(t), int(R))
    _check(min(n, 0), "hrn_tile_count")
    return n


def _window_range(w0, w1):
    w0, w1 = int(w0), int(w1)
    if not 0 <= w0 < w1:
        raise ValueError(f"the window range must satisfy 0 <= w0 < w1, got [{w0}, {w1})")
    return w0, w1


def tile_gather(lrs, t, R, w0, w1):
    """lrs (B,V,H,W) -> (w1-w0, B, V, t, t), window-major: the windows w0 <= w < w1 of tiling.plan(H, W, t, R), bit for bit
    tiling.gather(lrs, plan.windows[w0:w1], t).  One launch of hrn_tile_gather on the current stream."""
    lrs = _dev_f32(lrs, "lrs")
    if lrs.dim() != 4 or lrs.numel() == 0:
        raise ValueError(f"lrs must be a non-empty (B,V,H,W); got {tuple(lrs.shape)}")
    w0, w1 = _window_range(w0, w1)
    B, V, H, W = lrs.shape
    t = int(t)
    with torch.cuda.device(lrs.device):
        out = torch.empty((w1 - w0, B, V, max(t, 0), max(t, 0)), dtype=torch.float32, device=lrs.device)
        _check(load_library().hrn_tile_gather(_ptr(lrs), B, V, H, W, t, int(R), w0, w1, _ptr(out), _stream()), "hrn_tile_gather")
    return out


def tile_scatter(out, srs, t, R, scale, w0, w1):
    """srs (w1-w0, B, 1, S t, S t), the forwards of the windows w0 <= w < w1 of tiling.plan(H, W, t, R) -> their cores in
    out (B, 1, S H, S W), in place (contiguous float32 on srs's device); bit for bit tiling.scatter(out, srs, plan.windows[w0:w1], t,
    scale).  One launch of hrn_tile_scatter on the current stream."""
    srs = _dev_f32(srs, "srs")
    w0, w1 = _window_range(w0, w1)
    t, S = int(t), int(scale)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 \
            or out.shape[1] != 1 or out.device != srs.device or out.numel() == 0:
        raise ValueError("out must be a contiguous float32 (B, 1, S H, S W) tensor on srs's device")
    B = out.shape[0]
    if S not in SCALES or out.shape[2] % S or out.shape[3] % S:
        raise ValueError(f"scale must be one of {SCALES} and divide out's sides; got scale {scale!r} for out {tuple(out.shape)}")
    if tuple(srs.shape) != (w1 - w0, B, 1, S * t, S * t):
        raise ValueError(f"srs must be {(w1 - w0, B, 1, S * t, S * t)}; got {tuple(srs.shape)}")
    with torch.cuda.device(srs.device):
        _check(load_library().hrn_tile_scatter(_ptr(srs), B, out.shape[2] // S, out.shape[3] // S, t, int(R), S, w0, w1, _ptr(out), _stream()),
               "hrn_tile_scatter")
    return out


RESAMPLE_TAPS = 12        # HRN_RESAMPLE_TAPS: weights per output sample in a resampling table


def resample_targets(src, dst, jobs, n_in, n_out, table):
    """One launch on the current stream: every image of `jobs` - a host (n, 2) integer array of element offsets (source image in
    `src`, result in `dst`) - resampled from n_in x n_in to n_out x n_out.  src / dst: 1-D device tensors, both uint16 (HR images:
    fp64 sum, clip, round half to even) or both uint8 (status maps: clear only if every sample under a non-zero weight is clear).
    table = (first, count, weights) from hrnet_hip.resample.weight_table, host arrays.  Everything is checked here, before the
    launch (include/hrnet_hip.h, hrn_resample_targets)."""
    for name, t in (("src", src), ("dst", dst)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.dim() != 1 or t.dtype not in (torch.uint16, torch.uint8):
            raise RuntimeError(f"{name} must be a contiguous 1-D uint16 or uint8 ROCm device tensor")
    if src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError(f"src ({src.dtype}, {src.device}) and dst ({dst.dtype}, {dst.device}) must share dtype and device")
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0 or not any(n_in * s == n_out * r for r in (2, 3, 4) for s in (2, 3, 4)):
        raise ValueError(f"n_in : n_out must be R : S with R, S in {{2, 3, 4}}, got {n_in} : {n_out}")
    jobs = np.ascontiguousarray(jobs, dtype=np.int64)
    if jobs.ndim != 2 or jobs.shape[1] != 2 or not 0 < jobs.shape[0] <= 65535:
        raise ValueError(f"jobs must be (n, 2) with 1 <= n <= 65535, got {jobs.shape}")
    if jobs.min() < 0 or int(jobs[:, 0].max()) + n_in * n_in > src.numel() or int(jobs[:, 1].max()) + n_out * n_out > dst.numel():
        raise ValueError("jobs: an image lies outside src / dst")
    first, count, weights = (np.ascontiguousarray(a, dtype=dt) for a, dt in zip(table, (np.int32, np.int32, np.float64)))
    if first.shape != (n_out,) or count.shape != (n_out,) or weights.shape != (n_out, RESAMPLE_TAPS):
        raise ValueError(f"table must be first ({n_out},), count ({n_out},), weights ({n_out}, {RESAMPLE_TAPS})")
    if first.min() < 0 or count.min() < 1 or count.max() > RESAMPLE_TAPS or int((first.astype(np.int64) + count).max()) > n_in:
        raise ValueError("table: taps must lie inside the source image, 1..12 per output sample")
    if not np.isfinite(weights).all():
        raise ValueError("table: weights must be finite")
    with torch.cuda.device(src.device):
        dev = lambda a: torch.from_numpy(a).to(src.device)
        jobs_d, first_d, count_d, weights_d = dev(jobs), dev(first), dev(count), dev(weights)
        _check(load_library().hrn_resample_targets(_ptr(src), src.numel(), _ptr(dst), dst.numel(), src.element_size(), _ptr(jobs_d),
                                                   jobs.shape[0], n_in, n_out, _ptr(first_d), _ptr(count_d), _ptr(weights_d), _stream()),
               "hrn_resample_targets")
        for t in (jobs_d, first_d, count_d, weights_d):
            t.record_stream(torch.cuda.current_stream())


# --------------------------------------------------------------------------- built-in kernel timing
def profile_enable(on):
    _check(load_library().hrn_profile_enable(int(bool(on))), "hrn_profile_enable")


def profile_read():
    """-> {family: dict(launches, ms, flops, bytes)} for everything recorded since profile_enable(True)."""
    lib = load_library()
    out = {}
    for i in range(lib.hrn_profile_count()):
        name = ctypes.create_string_buffer(64)
        n, ms, fl, by = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(lib.hrn_profile_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)), "hrn_profile_get")
        out[name.value.decode()] = {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
    return out


# --------------------------------------------------------------------------- loss / score reductions
_METRICS = {"masked_MSE": 0, "cMSE": 1, "cPSNR": 2}


def get_loss(srs, hrs, hr_maps, metric="cMSE", crop=0):
    """get_loss of the reference (train.py:66-87) on device: (B,S,S) tensors -> (B,).  `crop` folds get_crop_mask in."""
    lib = load_library()
    if metric not in _METRICS:
        raise ValueError(f"metric must be one of {sorted(_METRICS)}; got {metric!r}")
    srs, hrs, hr_maps = _dev_f32(srs, "srs"), _dev_f32(hrs, "hrs"), _dev_f32(hr_maps, "hr_maps")
    if srs.dim() != 3 or srs.shape != hrs.shape or srs.shape != hr_maps.shape or srs.shape[1] != srs.shape[2]:
        raise ValueError(f"srs, hrs, hr_maps must be equal (B,S,S) tensors; got {tuple(srs.shape)}, {tuple(hrs.shape)}, {tuple(hr_maps.shape)}")
    B, S, _ = srs.shape
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_get_loss(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, S, int(crop), _METRICS[metric], _ptr(out), _stream()), "hrn_get_loss")
    return out


def get_loss_train(srs, hrs, hr_maps, metric="cPSNR", crop=0):
    """Forward of the differentiable loss tail: -> (out (B,), stats (B,4) f64 = {n, bias, cMSE, 0})."""
    lib = load_library()
    if metric not in ("cMSE", "cPSNR"):
        raise ValueError(f"the registered loss is defined for 'cMSE' and 'cPSNR'; got {metric!r}")
    srs, hrs, hr_maps = _dev_f32(srs, "srs"), _dev_f32(hrs, "hrs"), _dev_f32(hr_maps, "hr_maps")
    if srs.dim() != 3 or srs.shape != hrs.shape or srs.shape != hr_maps.shape or srs.shape[1] != srs.shape[2]:
        raise ValueError(f"srs, hrs, hr_maps must be equal (B,S,S) tensors; got {tuple(srs.shape)}, {tuple(hrs.shape)}, {tuple(hr_maps.shape)}")
    B, S, _ = srs.shape
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    stats = torch.empty((B, 4), dtype=torch.float64, device=srs.device)
    with torch.cuda.device(srs.device):
        ws = _workspace(lib.hrn_get_loss_train_workspace_bytes(B), srs.device, "loss_train")
        _check(lib.hrn_get_loss_train(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, S, int(crop), _METRICS[metric], _ptr(out), _ptr(stats),
                                      _ptr(ws), ws.numel(), _stream()), "hrn_get_loss_train")
    return out, stats


def get_loss_backward(srs, hrs, hr_maps, stats, d_out, metric="cPSNR", crop=0):
    """d_out (B,) -> d_srs (B,S,S): the brightness bias is a constant, as in the reference (train.py:83)."""
    lib = load_library()
    srs, hrs, hr_maps, d_out = _dev_f32(srs, "srs"), _dev_f32(hrs, "hrs"), _dev_f32(hr_maps, "hr_maps"), _dev_f32(d_out, "d_out")
    B, S, _ = srs.shape
    d_srs = torch.empty_like(srs)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_get_loss_backward(_ptr(srs), _ptr(hrs), _ptr(hr_maps), _ptr(stats), _ptr(d_out), B, S, int(crop),
                                         _METRICS[metric], _ptr(d_srs), _stream()), "hrn_get_loss_backward")
    return d_srs


def shift_cpsnr(srs, hrs, hr_maps, border_w=3, clip=True):
    """Batched shift_cPSNR (Evaluator.py:52-73) on device: (B,S,S) tensors -> (B,) best cPSNR over the (2w+1)^2 offsets."""
    lib = load_library()
    srs, hrs, hr_maps = _dev_f32(srs, "srs"), _dev_f32(hrs, "hrs"), _dev_f32(hr_maps, "hr_maps")
    if srs.dim() == 2:
        srs, hrs, hr_maps = srs[None], hrs[None], hr_maps[None]
    if srs.dim() != 3 or srs.shape != hrs.shape or srs.shape != hr_maps.shape or srs.shape[1] != srs.shape[2]:
        raise ValueError("srs, hrs, hr_maps must be equal (B,S,S) tensors")
    B, S, _ = srs.shape
    nws = lib.hrn_shift_cpsnr_workspace_bytes(B, int(border_w))
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    with torch.cuda.device(srs.device):
        ws = _workspace(nws, srs.device, "shift_cpsnr")
        _check(lib.hrn_shift_cpsnr(_ptr(srs.contiguous()), _ptr(hrs.contiguous()), _ptr(hr_maps.contiguous()), B, S, int(border_w),
                                   int(bool(clip)), _ptr(out), _ptr(ws), ws.numel(), _stream()), "hrn_shift_cpsnr")
    return out


def _bhw_frames(srs, hrs, hr_maps):
    """the frame check of the searched losses and scores -> three dense f32 device tensors of equal (B,H,W) shapes"""
    srs, hrs, hr_maps = _dev_f32(srs, "srs"), _dev_f32(hrs, "hrs"), _dev_f32(hr_maps, "hr_maps")
    if srs.dim() != 3 or srs.shape != hrs.shape or srs.shape != hr_maps.shape:
        raise ValueError(f"srs, hrs, hr_maps must be equal (B,H,W) tensors; got {tuple(srs.shape)}, {tuple(hrs.shape)}, {tuple(hr_maps.shape)}")
    return srs, hrs, hr_maps


def _shift_loss_args(srs, hrs, hr_maps, metric, border_w):
    if metric not in ("cMSE", "cPSNR"):
        raise ValueError(f"the searched loss is defined for 'cMSE' and 'cPSNR'; got {metric!r}")
    srs, hrs, hr_maps = _bhw_frames(srs, hrs, hr_maps)
    border_w = int(border_w)
    if border_w < 0 or min(srs.shape[1:]) <= 2 * border_w:
        raise ValueError(f"border_w={border_w} needs frames larger than {2 * border_w} pixels each way; got {tuple(srs.shape[1:])}")
    return srs, hrs, hr_maps, border_w


def shift_loss_train(srs, hrs, hr_maps, metric="cPSNR", border_w=3, clip=False):
    """Forward of the shift-searched loss (Evaluator.py:52-73 over train.py:66-87) on (B,H,W) frames of any aspect ratio: -> (out (B,),
    stats (B,4) f64 = {n, bias, cMSE, k} of the selected offset k = u (2 border_w + 1) + v)."""
    lib = load_library()
    srs, hrs, hr_maps, border_w = _shift_loss_args(srs, hrs, hr_maps, metric, border_w)
    B, H, W = srs.shape
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    stats = torch.empty((B, 4), dtype=torch.float64, device=srs.device)
    with torch.cuda.device(srs.device):
        ws = _workspace(lib.hrn_shift_loss_workspace_bytes(B, H, W, border_w), srs.device, "shift_loss")
        _check(lib.hrn_shift_loss_train(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, H, W, border_w, _METRICS[metric], int(bool(clip)), _ptr(out),
                                        _ptr(stats), _ptr(ws), ws.numel(), _stream()), "hrn_shift_loss_train")
    return out, stats


def shift_loss_backward(srs, hrs, hr_maps, stats, d_out, metric="cPSNR", border_w=3, clip=False):
    """d_out (B,) -> d_srs (B,H,W) through the offset `stats` selected; zero on the border frame and where clip clamped."""
    lib = load_library()
    srs, hrs, hr_maps, border_w = _shift_loss_args(srs, hrs, hr_maps, metric, border_w)
    d_out = _dev_f32(d_out, "d_out")
    B, H, W = srs.shape
    if tuple(stats.shape) != (B, 4) or stats.dtype != torch.float64 or tuple(d_out.shape) != (B,):
        raise ValueError(f"stats must be ({B}, 4) float64 and d_out ({B},); got {tuple(stats.shape)} {stats.dtype}, {tuple(d_out.shape)}")
    d_srs = torch.empty_like(srs)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_shift_loss_backward(_ptr(srs), _ptr(hrs), _ptr(hr_maps), _ptr(stats.contiguous()), _ptr(d_out), B, H, W, border_w,
                                           _METRICS[metric], int(bool(clip)), _ptr(d_srs), _stream()), "hrn_shift_loss_backward")
    return d_srs


def _cl1_loss_args(srs, hrs, hr_maps, border_w, eps):
    srs, hrs, hr_maps = _bhw_frames(srs, hrs, hr_maps)
    border_w, eps = int(border_w), float(eps)
    if border_w < 0 or min(srs.shape[1:]) <= 2 * border_w:
        raise ValueError(f"border_w={border_w} needs frames larger than {2 * border_w} pixels each way; got {tuple(srs.shape[1:])}")
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be finite and not negative; got {eps}")
    return srs, hrs, hr_maps, border_w, eps


def cl1_loss_train(srs, hrs, hr_maps, border_w=3, clip=False, eps=0.0):
    """Forward of the shift-searched, brightness-corrected L1 (eps == 0) / Charbonnier loss on (B,H,W) frames of any
    aspect ratio: -> (out (B,), stats (B,5) f64 = {n, bias, cL1, k, sigma} of the selected offset k = u (2 border_w + 1) + v)."""
    lib = load_library()
    srs, hrs, hr_maps, border_w, eps = _cl1_loss_args(srs, hrs, hr_maps, border_w, eps)
    B, H, W = srs.shape
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    stats = torch.empty((B, 5), dtype=torch.float64, device=srs.device)
    with torch.cuda.device(srs.device):
        ws = _workspace(lib.hrn_cl1_loss_workspace_bytes(B, H, W, border_w), srs.device, "cl1_loss")
        _check(lib.hrn_cl1_loss_train(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, H, W, border_w, int(bool(clip)), eps, _ptr(out), _ptr(stats),
                                      _ptr(ws), ws.numel(), _stream()), "hrn_cl1_loss_train")
    return out, stats


def cl1_loss_backward(srs, hrs, hr_maps, stats, d_out, border_w=3, clip=False, eps=0.0):
    """d_out (B,) -> d_srs (B,H,W) through the offset `stats` selected, the bias attached; zero on the border frame and where clip
    clamped."""
    lib = load_library()
    srs, hrs, hr_maps, border_w, eps = _cl1_loss_args(srs, hrs, hr_maps, border_w, eps)
    d_out = _dev_f32(d_out, "d_out")
    B, H, W = srs.shape
    if tuple(stats.shape) != (B, 5) or stats.dtype != torch.float64 or tuple(d_out.shape) != (B,):
        raise ValueError(f"stats must be ({B}, 5) float64 and d_out ({B},); got {tuple(stats.shape)} {stats.dtype}, {tuple(d_out.shape)}")
    d_srs = torch.empty_like(srs)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_cl1_loss_backward(_ptr(srs), _ptr(hrs), _ptr(hr_maps), _ptr(stats.contiguous()), _ptr(d_out), B, H, W, border_w,
                                         int(bool(clip)), eps, _ptr(d_srs), _stream()), "hrn_cl1_loss_backward")
    return d_srs


SUBPIXEL_STATS = 8        # hrn_subpixel_loss_train's stats: n*, b*, cMSE*, dy*, dx*, mean sr, mean hr under m0, centred bias


def _subpixel_loss_args(srs, hrs, hr_maps, metric, border_w):
    """the frames, the metric and the border of the sub-pixel searched loss; the search's own limits are mncc_int's"""
    if metric not in ("cMSE", "cPSNR"):
        raise ValueError(f"the searched loss is defined for 'cMSE' and 'cPSNR'; got {metric!r}")
    srs, hrs, hr_maps = _bhw_frames(srs, hrs, hr_maps)
    border_w = int(border_w)
    if border_w < 0 or border_w > 8 or min(srs.shape[1:]) <= 2 * border_w:
        raise ValueError(f"border_w must be 0..8 and smaller than half of each side; got {border_w} for frames {tuple(srs.shape[1:])}")
    return srs, hrs, hr_maps, border_w


def _subpixel_workspace(B, H, W, P, device):
    # MNCC_POINTS is defined with the registration wrappers below; this runs after the module is loaded
    return _mncc_workspace("hrn_subpixel_loss_workspace_bytes", (B, H, W, P), "subpixel_loss", f"B={B} H={H} W={W} P={P}", device)


def subpixel_loss_train(srs, hrs, hr_maps, metric="cPSNR", border_w=3, points_per_dim=7, levels=4, radius=3.0):
    """Forward of the sub-pixel searched loss on (B,H,W) frames: -> (out (B,), stats (B,8) f64 = {n*, b*, cMSE*,
    dy*, dx*, mean sr, mean hr, centred bias} at the point s* = (dy*, dx*) the search found, trace (B,levels,3) f32 = (dy, dx, cMSE) of
    every level's point)."""
    lib = load_library()
    srs, hrs, hr_maps, border_w = _subpixel_loss_args(srs, hrs, hr_maps, metric, border_w)
    P, levels = mncc_int("points_per_dim", points_per_dim, MNCC_POINTS), mncc_int("levels", levels, MNCC_LEVELS)
    B, H, W = srs.shape
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    stats = torch.empty((B, SUBPIXEL_STATS), dtype=torch.float64, device=srs.device)
    trace = torch.empty((B, levels, 3), dtype=torch.float32, device=srs.device)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_subpixel_loss_train(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, H, W, border_w, P, levels, float(radius), _METRICS[metric],
                                           _ptr(out), _ptr(stats), _ptr(trace), *_subpixel_workspace(B, H, W, P, srs.device), _stream()),
               "hrn_subpixel_loss_train")
    return out, stats, trace


def subpixel_loss_backward(srs, hrs, hr_maps, stats, d_out, metric="cPSNR", border_w=3):
    """d_out (B,) -> d_srs (B,H,W): the sampler's adjoint, at the point `stats` holds, of the residual's gradient; every element written,
    exactly zero where no counted pixel's footprint reaches."""
    lib = load_library()
    srs, hrs, hr_maps, border_w = _subpixel_loss_args(srs, hrs, hr_maps, metric, border_w)
    d_out = _dev_f32(d_out, "d_out")
    B, H, W = srs.shape
    if tuple(stats.shape) != (B, SUBPIXEL_STATS) or stats.dtype != torch.float64 or tuple(d_out.shape) != (B,):
        raise ValueError(f"stats must be ({B}, {SUBPIXEL_STATS}) float64 and d_out ({B},); got {tuple(stats.shape)} {stats.dtype}, "
                         f"{tuple(d_out.shape)}")
    d_srs = torch.empty_like(srs)
    with torch.cuda.device(srs.device):
        _check(lib.hrn_subpixel_loss_backward(_ptr(srs), _ptr(hrs), _ptr(hr_maps), _ptr(stats.contiguous()), _ptr(d_out), B, H, W, border_w,
                                              _METRICS[metric], _ptr(d_srs), *_subpixel_workspace(B, H, W, MNCC_POINTS[0], srs.device),
                                              _stream()), "hrn_subpixel_loss_backward")
    return d_srs


CSSIM_WINDOWS = {"gaussian": (0, 11), "uniform": (1, 7)}      # name -> (hrn_shift_cssim's `window`, taps)


def _cssim_args(srs, hrs, hr_maps, border_w, window, data_range):
    """the checks of the cSSIM entry points -> (srs, hrs, hr_maps as dense f32, border_w, hrn_shift_cssim's window code, data_range)"""
    if window not in CSSIM_WINDOWS:
        raise ValueError(f"window must be one of {sorted(CSSIM_WINDOWS)}; got {window!r}")
    code, taps = CSSIM_WINDOWS[window]
    srs, hrs, hr_maps = _bhw_frames(srs, hrs, hr_maps)
    border_w, data_range = int(border_w), float(data_range)
    if border_w < 0 or border_w > 8 or min(srs.shape[1:]) < 2 * border_w + taps:
        raise ValueError(f"border_w must be 0..8 and each side at least 2 border_w + {taps} (the {window} window); got {border_w} for "
                         f"frames {tuple(srs.shape[1:])}")
    if not data_range > 0.0:
        raise ValueError(f"data_range must be positive; got {data_range}")
    return srs, hrs, hr_maps, border_w, code, data_range


def shift_cssim(srs, hrs, hr_maps, border_w=3, window="gaussian", clip=True, correct_bias=True, data_range=1.0, with_scores=True):
    """The shift-searched, brightness-corrected SSIM (include/hrnet_hip.h) on (B,H,W) frames: -> (out (B,) f32,
    stats (B,4) f64 = {n, bias, score, k} of the selected offset k = u (2 border_w + 1) + v, scores (B, (2 border_w + 1)^2) f64 =
    the score of every offset, -inf where an offset has no clear pixel).  with_scores=False: scores = NULL to the same kernels, and
    None here."""
    lib = load_library()
    srs, hrs, hr_maps, border_w, code, data_range = _cssim_args(srs, hrs, hr_maps, border_w, window, data_range)
    B, H, W = srs.shape
    nk = (2 * border_w + 1) ** 2
    out = torch.empty((B,), dtype=torch.float32, device=srs.device)
    stats = torch.empty((B, 4), dtype=torch.float64, device=srs.device)
    scores = torch.empty((B, nk), dtype=torch.float64, device=srs.device) if with_scores else None
    with torch.cuda.device(srs.device):
        ws = _workspace(lib.hrn_shift_cssim_workspace_bytes(B, H, W, border_w, code), srs.device, "shift_cssim")
        _check(lib.hrn_shift_cssim(_ptr(srs), _ptr(hrs), _ptr(hr_maps), B, H, W, border_w, code, int(bool(clip)), int(bool(correct_bias)),
                                   data_range, _ptr(out), _ptr(stats), _ptr(scores) if with_scores else None, _ptr(ws), ws.numel(),
                                   _stream()), "hrn_shift_cssim")
    return out, stats, scores


def cssim_loss_backward(srs, hrs, hr_maps, stats, d_out, border_w=3, window="gaussian", clip=False, correct_bias=True, data_range=1.0):
    """d_out (B,) -> d_srs (B,H,W): d_out[b] times the gradient of the cSSIM score through the offset `stats` selected, the bias attached
    (include/hrnet_hip.h); zero on the border frame, on masked pixels, where clip clamped and for a sample without
    an eligible offset."""
    lib = load_library()
    srs, hrs, hr_maps, border_w, code, data_range = _cssim_args(srs, hrs, hr_maps, border_w, window, data_range)
    d_out = _dev_f32(d_out, "d_out")
    B, H, W = srs.shape
    if tuple(stats.shape) != (B, 4) or stats.dtype != torch.float64 or tuple(d_out.shape) != (B,):
        raise ValueError(f"stats must be ({B}, 4) float64 and d_out ({B},); got {tuple(stats.shape)} {stats.dtype}, {tuple(d_out.shape)}")
    d_srs = torch.empty_like(srs)
    with torch.cuda.device(srs.device):
        ws = _workspace(lib.hrn_cssim_loss_backward_workspace_bytes(B, H, W, border_w, code), srs.device, "cssim_loss_backward")
        _check(lib.hrn_cssim_loss_backward(_ptr(srs), _ptr(hrs), _ptr(hr_maps), _ptr(stats.contiguous()), _ptr(d_out), B, H, W, border_w,
                                           code, int(bool(clip)), int(bool(correct_bias)), data_range, _ptr(d_srs), _ptr(ws), ws.numel(),
                                           _stream()), "hrn_cssim_loss_backward")
    return d_srs


# --------------------------------------------------------------------------- sub-pixel registration of LR views.  Four files, one per
# path: registration.hip (frames that fit one CU's LDS), registration_scene.hip (frames of any size, in tiles), registration_local.hip (a
# shift per block of tiles: a field) and registration_pyramid.hip (coarse to fine, for shifts beyond 4 px).  grid / search / apply have a
# `scene` form that differs in the entry point, in the workspace it takes from the cache and in the limit on a frame's side, nothing
# else.  The tensor checks (_mncc_views, _mncc_args, _mncc_init) and the workspace (_mncc_workspace) are shared by all four.
MNCC_SIDES, MNCC_POINTS, MNCC_LEVELS, MNCC_MAX_RADIUS = (16, 128), (3, 9), (1, 16), 4.0     # the limits of include/hrnet_hip.h
MNCC_SCENE_SIDES = (16, 16384)
MNCC_LOCAL_BLOCKS = (64, 4096)             # a block of the local search: a multiple of 64 within these
MNCC_REDUCE_SIDES = (32, 16384)            # a plane reduce2 takes
MNCC_OCTAVES, MNCC_PYRAMID_MAX_REACH = (0, 6), 128.0       # of the pyramid search; radius * 2^octaves in pixels of the frame


def mncc_int(name, value, limits):
    value = int(value)
    if not limits[0] <= value <= limits[1]:
        raise ValueError(f"{name} must be {limits[0]}..{limits[1]}; got {value}")
    return value


def _mncc_views(views, view_masks, ref=None):
    """-> views (B,V,H,W) and view_masks (None: all ones) as contiguous device f32; with `ref`, views must be V frames of its shape."""
    views = _dev_f32(views, "views")
    if ref is None:
        if views.dim() != 4:
            raise ValueError(f"views must be (B,V,H,W); got {tuple(views.shape)}")
    elif views.dim() != 4 or ref.dim() != 3 or tuple(ref.shape) != (views.shape[0],) + tuple(views.shape[2:]):
        raise ValueError(f"ref must be (B,H,W) and views (B,V,H,W); got {tuple(ref.shape)}, {tuple(views.shape)}")
    if view_masks is not None:
        view_masks = _dev_f32(view_masks, "view_masks")
        if view_masks.shape != views.shape:
            raise ValueError(f"view_masks must have views' shape {tuple(views.shape)}; got {tuple(view_masks.shape)}")
    return views, view_masks


def _mncc_args(ref, ref_mask, views, view_masks):
    """-> the four tensors as contiguous device f32 (a mask may be None: all ones) after the shape checks."""
    ref = _dev_f32(ref, "ref")
    views, view_masks = _mncc_views(views, view_masks, ref)
    if ref_mask is not None:
        ref_mask = _dev_f32(ref_mask, "ref_mask")
        if ref_mask.shape != ref.shape:
            raise ValueError(f"ref_mask must have ref's shape {tuple(ref.shape)}; got {tuple(ref_mask.shape)}")
    return ref, ref_mask, views, view_masks


def _mncc_init(init, B, V):
    if init is not None:
        init = _dev_f32(init, "init")
        if tuple(init.shape) != (B, V, 2):
            raise ValueError(f"init must be ({B}, {V}, 2); got {tuple(init.shape)}")
    return init


def _opt_ptr(t):
    return ctypes.c_void_p(0) if t is None else _ptr(t)


def _mncc_workspace(query, args, tag, problem, device):
    """-> the (pointer, bytes) pair of an entry point's workspace arguments, from the cache under `tag`.  `query`(*args) is the entry
    point's size query: 0 where the entry point would refuse the `problem`.  The caller is inside torch.cuda.device(device)."""
    nbytes = getattr(load_library(), query)(*args)
    if nbytes == 0:
        raise HrnetHipError(f"bad registration problem size {problem}")
    ws = _workspace(nbytes, device, tag)
    return _ptr(ws), ws.numel()


def _mncc_scene_workspace(B, V, H, W, P, device):
    return _mncc_workspace("hrn_mncc_scene_workspace_bytes", (B, V, H, W, P), "mncc_scene", f"B={B} V={V} H={H} W={W} P={P}", device)


def _mncc_grid(scene, ref, ref_mask, views, view_masks, centres, points_per_dim, width):
    lib = load_library()
    ref, ref_mask, views, view_masks = _mncc_args(ref, ref_mask, views, view_masks)
    B, V, H, W = views.shape
    centres = _dev_f32(centres, "centres")
    if tuple(centres.shape) != (B, V, 2):
        raise ValueError(f"centres must be ({B}, {V}, 2); got {tuple(centres.shape)}")
    P = mncc_int("points_per_dim", points_per_dim, MNCC_POINTS)
    scores = torch.empty((B, V, P, P), dtype=torch.float32, device=views.device)
    args = (_ptr(ref), _opt_ptr(ref_mask), _ptr(views), _opt_ptr(view_masks), _ptr(centres), B, V, H, W, P, float(width), _ptr(scores))
    with torch.cuda.device(views.device):
        if scene:
            _check(lib.hrn_mncc_grid_scene(*args, *_mncc_scene_workspace(B, V, H, W, P, views.device), _stream()), "hrn_mncc_grid_scene")
        else:
            _check(lib.hrn_mncc_grid(*args, _stream()), "hrn_mncc_grid")
    return scores


def _mncc_search(entry, ref, ref_mask, views, view_masks, points_per_dim, levels, radius, init=None):
    """`entry`: hrn_mncc_search, hrn_mncc_search_scene or hrn_mncc_search_scene_from - the one that takes `init`."""
    lib = load_library()
    ref, ref_mask, views, view_masks = _mncc_args(ref, ref_mask, views, view_masks)
    B, V, H, W = views.shape
    P, levels = mncc_int("points_per_dim", points_per_dim, MNCC_POINTS), mncc_int("levels", levels, MNCC_LEVELS)
    init = _mncc_init(init, B, V)
    shifts = torch.empty((B, V, 2), dtype=torch.float32, device=views.device)
    trace = torch.empty((B, V, levels, 3), dtype=torch.float32, device=views.device)
    args = [_ptr(ref), _opt_ptr(ref_mask), _ptr(views), _opt_ptr(view_masks)]
    if entry == "hrn_mncc_search_scene_from":
        args.append(_opt_ptr(init))
    args += [B, V, H, W, P, levels, float(radius), _ptr(shifts), _ptr(trace)]
    with torch.cuda.device(views.device):
        if entry != "hrn_mncc_search":
            args += _mncc_scene_workspace(B, V, H, W, P, views.device)
        _check(getattr(lib, entry)(*args, _stream()), entry)
    return shifts, trace


def _mncc_apply(scene, views, view_masks, shifts):
    lib = load_library()
    views, view_masks = _mncc_views(views, view_masks)
    B, V, H, W = views.shape
    shifts = _dev_f32(shifts, "shifts")
    if tuple(shifts.shape) != (B, V, 2):
        raise ValueError(f"shifts must be ({B}, {V}, 2); got {tuple(shifts.shape)}")
    out, valid = torch.empty_like(views), torch.empty_like(views)
    name = "hrn_mncc_apply_scene" if scene else "hrn_mncc_apply"
    with torch.cuda.device(views.device):
        _check(getattr(lib, name)(_ptr(views), _opt_ptr(view_masks), _ptr(shifts), B, V, H, W, _ptr(out), _ptr(valid), _stream()), name)
    return out, valid


def mncc_grid(ref, ref_mask, views, view_masks, centres, points_per_dim, width):
    """One level of the masked-NCC search (include/hrnet_hip.h): centres (B,V,2) = (cy, cx) -> scores (B,V,P,P) f32 for the grid points
    (dy_i, dx_j) of `width` around them.  A mask may be None (all ones)."""
    return _mncc_grid(False, ref, ref_mask, views, view_masks, centres, points_per_dim, width)


def mncc_search(ref, ref_mask, views, view_masks, points_per_dim=7, levels=6, radius=1.0):
    """The whole search in one launch: -> (shifts (B,V,2) f32 = (dy, dx), trace (B,V,levels,3) f32 = (dy, dx, score) per level)."""
    return _mncc_search("hrn_mncc_search", ref, ref_mask, views, view_masks, points_per_dim, levels, radius)


def mncc_apply(views, view_masks, shifts):
    """-> (out (B,V,H,W) = S(view, shift), valid (B,V,H,W) f32 0 / 1 = V(mask, shift)); invalid pixels of `out` are 0."""
    return _mncc_apply(False, views, view_masks, shifts)


def mncc_grid_scene(ref, ref_mask, views, view_masks, centres, points_per_dim, width):
    """mncc_grid for frames of any size (hrn_mncc_grid_scene): tiles, a workspace from the cache, the same scores."""
    return _mncc_grid(True, ref, ref_mask, views, view_masks, centres, points_per_dim, width)


def mncc_search_scene(ref, ref_mask, views, view_masks, points_per_dim=7, levels=6, radius=1.0):
    """mncc_search for frames of any size (hrn_mncc_search_scene): 1 + 2 levels launches, nothing returns to the host between them."""
    return _mncc_search("hrn_mncc_search_scene", ref, ref_mask, views, view_masks, points_per_dim, levels, radius)


def mncc_apply_scene(views, view_masks, shifts):
    """mncc_apply for frames of any size (hrn_mncc_apply_scene); bit-identical to it where both run."""
    return _mncc_apply(True, views, view_masks, shifts)


def mncc_apply_backward(views, shifts, valid, d_out, need_views=True, need_shifts=True):
    """The backward of mncc_apply_scene (hrn_mncc_apply_backward): valid = its second result, d_out = the gradient at its first ->
    (d_views (B,V,H,W) or None, d_shifts (B,V,2) or None), each computed only where needed; both unneeded is an error.  The gradient
    takes d_out where `valid` is set and the pixel's footprint lies inside the frame.  Bit-reproducible."""
    if not (need_views or need_shifts):
        raise ValueError("mncc_apply_backward: neither d_views nor d_shifts is needed")
    lib = load_library()
    views, _ = _mncc_views(views, None)
    B, V, H, W = views.shape
    shifts, valid, d_out = _dev_f32(shifts, "shifts"), _dev_f32(valid, "valid"), _dev_f32(d_out, "d_out")
    if tuple(shifts.shape) != (B, V, 2):
        raise ValueError(f"shifts must be ({B}, {V}, 2); got {tuple(shifts.shape)}")
    for name, t in (("valid", valid), ("d_out", d_out)):
        if t.shape != views.shape:
            raise ValueError(f"{name} must have views' shape {tuple(views.shape)}; got {tuple(t.shape)}")
    d_views = torch.empty_like(views) if need_views else None
    d_shifts = torch.empty((B, V, 2), dtype=torch.float32, device=views.device) if need_shifts else None
    with torch.cuda.device(views.device):
        ws = (ctypes.c_void_p(0), 0)
        if need_shifts:
            ws = _mncc_workspace("hrn_mncc_apply_backward_workspace_bytes", (B, V, H, W), "mncc_apply_backward", f"B={B} V={V} H={H} W={W}",
                                 views.device)
        _check(lib.hrn_mncc_apply_backward(_ptr(views), _ptr(shifts), _ptr(valid), _ptr(d_out), B, V, H, W, _opt_ptr(d_views),
                                           _opt_ptr(d_shifts), *ws, _stream()), "hrn_mncc_apply_backward")
    return d_views, d_shifts


def mncc_search_scene_from(ref, ref_mask, views, view_masks, init, points_per_dim=7, levels=6, radius=1.0):
    """mncc_search_scene with the first level's centre read from init (B,V,2) (hrn_mncc_search_scene_from); None: (0, 0)."""
    return _mncc_search("hrn_mncc_search_scene_from", ref, ref_mask, views, view_masks, points_per_dim, levels, radius, init)


def mncc_reduce2(x, mask):
    """x (N,H,W), mask (N,H,W) or None (all clear) -> (out (N,H//2,W//2), out_mask f32 1 / 0): the masked [1, 3, 3, 1] / 8 reduction of
    include/hrnet_hip.h (hrn_mncc_reduce2)."""
    lib = load_library()
    x = _dev_f32(x, "x")
    if x.dim() != 3:
        raise ValueError(f"x must be (N,H,W); got {tuple(x.shape)}")
    if mask is not None:
        mask = _dev_f32(mask, "mask")
        if mask.shape != x.shape:
            raise ValueError(f"mask must have x's shape {tuple(x.shape)}; got {tuple(mask.shape)}")
    N, H, W = x.shape
    out = torch.empty((N, H // 2, W // 2), dtype=torch.float32, device=x.device)
    out_mask = torch.empty_like(out)
    with torch.cuda.device(x.device):
        _check(lib.hrn_mncc_reduce2(_ptr(x), _opt_ptr(mask), N, H, W, _ptr(out), _ptr(out_mask), _stream()), "hrn_mncc_reduce2")
    return out, out_mask


def mncc_search_pyramid(ref, ref_mask, views, view_masks, octaves=2, points_per_dim=7, levels=6, radius=4.0, coarse_levels=3, refine_radius=1.0):
    """The coarse-to-fine search (hrn_mncc_search_pyramid): -> (shifts (B,V,2) f32 in pixels of the frame, trace (B,V,octaves+1,3) f32 =
    (dy, dx, score) of every octave's last level in that octave's pixels, coarsest first)."""
    lib = load_library()
    ref, ref_mask, views, view_masks = _mncc_args(ref, ref_mask, views, view_masks)
    B, V, H, W = views.shape
    P, levels = mncc_int("points_per_dim", points_per_dim, MNCC_POINTS), mncc_int("levels", levels, MNCC_LEVELS)
    coarse_levels, K = mncc_int("coarse_levels", coarse_levels, MNCC_LEVELS), mncc_int("octaves", octaves, MNCC_OCTAVES)
    shifts = torch.empty((B, V, 2), dtype=torch.float32, device=views.device)
    trace = torch.empty((B, V, K + 1, 3), dtype=torch.float32, device=views.device)
    with torch.cuda.device(views.device):
        ws = _mncc_workspace("hrn_mncc_pyramid_workspace_bytes", (B, V, H, W, P, K), "mncc_pyramid",
                             f"B={B} V={V} H={H} W={W} P={P} octaves={K}", views.device)
        _check(lib.hrn_mncc_search_pyramid(_ptr(ref), _opt_ptr(ref_mask), _ptr(views), _opt_ptr(view_masks), B, V, H, W, P, K, levels,
                                           float(radius), coarse_levels, float(refine_radius), _ptr(shifts), _ptr(trace), *ws, _stream()),
               "hrn_mncc_search_pyramid")
    return shifts, trace


def mncc_block(block):
    """The side of a block of the local search as the library takes it: a multiple of 64 in 64..4096."""
    block = int(block)
    if not MNCC_LOCAL_BLOCKS[0] <= block <= MNCC_LOCAL_BLOCKS[1] or block % 64:
        raise ValueError(f"block must be a multiple of 64 in {MNCC_LOCAL_BLOCKS[0]}..{MNCC_LOCAL_BLOCKS[1]}; got {block}")
    return block


def mncc_local_blocks(H, W, block):
    """-> (by, bx): the blocks of an (H, W) frame, by hrn_mncc_local_blocks - the library's own count, not a restatement of it."""
    lib = load_library()
    block = mncc_block(block)
    by, bx = lib.hrn_mncc_local_blocks(int(H), block), lib.hrn_mncc_local_blocks(int(W), block)
    if by == 0 or bx == 0:
        raise ValueError(f"frames must be 1..{MNCC_SCENE_SIDES[1]} pixels a side; got {(int(H), int(W))}")
    return by, bx


def mncc_search_local(ref, ref_mask, views, view_masks, init, points_per_dim=7, levels=4, radius=0.5, block=128, min_valid=0.25):
    """A shift per block of every view (hrn_mncc_search_local): init (B,V,2) or None (zeros) -> (field (B,V,by,bx,2) f32, trace
    (B,V,by,bx,levels,3) f32 = (dy, dx, score) per level, ok (B,V,by,bx) f32 1 / 0); a block that is not ok holds init."""
    lib = load_library()
    ref, ref_mask, views, view_masks = _mncc_args(ref, ref_mask, views, view_masks)
    B, V, H, W = views.shape
    init = _mncc_init(init, B, V)
    P, levels = mncc_int("points_per_dim", points_per_dim, MNCC_POINTS), mncc_int("levels", levels, MNCC_LEVELS)
    by, bx = mncc_local_blocks(H, W, block)
    field = torch.empty((B, V, by, bx, 2), dtype=torch.float32, device=views.device)
    trace = torch.empty((B, V, by, bx, levels, 3), dtype=torch.float32, device=views.device)
    ok = torch.empty((B, V, by, bx), dtype=torch.float32, device=views.device)
    with torch.cuda.device(views.device):
        ws = _mncc_workspace("hrn_mncc_local_workspace_bytes", (B, V, H, W, P, int(block)), "mncc_local",
                             f"B={B} V={V} H={H} W={W} P={P} block={block}", views.device)
        _check(lib.hrn_mncc_search_local(_ptr(ref), _opt_ptr(ref_mask), _ptr(views), _opt_ptr(view_masks), _opt_ptr(init), B, V, H, W, P, levels,
                                         float(radius), int(block), float(min_valid), _ptr(field), _ptr(trace), _ptr(ok), *ws, _stream()),
               "hrn_mncc_search_local")
    return field, trace, ok


def mncc_apply_field(views, view_masks, field, block):
    """-> (out, valid) as mncc_apply_scene, every pixel by its own shift: the field (B,V,by,bx,2) between the blocks' centres."""
    lib = load_library()
    views, view_masks = _mncc_views(views, view_masks)
    B, V, H, W = views.shape
    field = _dev_f32(field, "field")
    by, bx = mncc_local_blocks(H, W, block)
    if tuple(field.shape) != (B, V, by, bx, 2):
        raise ValueError(f"field must be ({B}, {V}, {by}, {bx}, 2); got {tuple(field.shape)}")
    out, valid = torch.empty_like(views), torch.empty_like(views)
    with torch.cuda.device(views.device):
        _check(lib.hrn_mncc_apply_field(_ptr(views), _opt_ptr(view_masks), _ptr(field), B, V, H, W, int(block), _ptr(out), _ptr(valid),
                                        _stream()), "hrn_mncc_apply_field")
    return out, valid


# --------------------------------------------------------------------------- cloud-free composite reference frame
COMPOSITE_MAX_REF = 32    # hrn_masked_composite: 1 <= n_ref <= 32


def masked_composite(lrs, lr_masks=None, alphas=None, n_ref=9, want_count=False, fill=True):
    """hrn_masked_composite on contiguous f32 device tensors (hrnet_hip/composite.py checks them): -> (ref (B,H,W), filled (B,V,H,W) or
    None, count (B,H,W) or None)."""
    lib = load_library()
    B, V, H, W = lrs.shape
    ref = torch.empty((B, H, W), dtype=torch.float32, device=lrs.device)
    filled = torch.empty((B, V, H, W), dtype=torch.float32, device=lrs.device) if fill else None
    count = torch.empty((B, H, W), dtype=torch.float32, device=lrs.device) if want_count else None
    with torch.cuda.device(lrs.device):
        _check(lib.hrn_masked_composite(_ptr(lrs), _opt_ptr(lr_masks), _opt_ptr(alphas), B, V, H, W, int(n_ref), _ptr(ref), _opt_ptr(count),
                                        _opt_ptr(filled), _stream()), "hrn_masked_composite")
    return ref, filled, count


# --------------------------------------------------------------------------- bicubic upsampling (the global residual's frame)
UPSAMPLE_TILE = (8, 32)       # HRN_UPSAMPLE_TILE_H x HRN_UPSAMPLE_TILE_W: the LR pixels a workgroup of either kernel owns
UPSAMPLE_MAX_SIDE = 16384     # hrn_upsample: planes of 1 .. 16384 a side


def upsample(frames, base, scale, a, out=None):
    """hrn_upsample on contiguous f32 device tensors (hrnet_hip/upsample.py checks them): frames (N,H,W), base (N,SH,SW) or None ->
    out (N,SH,SW) = base + up(frames).  out: where the result goes (a new tensor when None); base may be out itself."""
    lib = load_library()
    N, H, W = frames.shape
    if out is None:
        out = torch.empty((N, scale * H, scale * W), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _check(lib.hrn_upsample(_ptr(frames), _opt_ptr(base), _ptr(out), N, H, W, int(scale), float(a), _stream()), "hrn_upsample")
    return out


def upsample_backward(d_out, H, W, scale, a):
    """hrn_upsample_backward: d_out (N,SH,SW) contiguous f32 -> d_frames (N,H,W) = the adjoint of up() applied to d_out."""
    lib = load_library()
    N = d_out.shape[0]
    d_frames = torch.empty((N, H, W), dtype=torch.float32, device=d_out.device)
    with torch.cuda.device(d_out.device):
        _check(lib.hrn_upsample_backward(_ptr(d_out), _ptr(d_frames), N, int(H), int(W), int(scale), float(a), _stream()),
               "hrn_upsample_backward")
    return d_frames


# --------------------------------------------------------------------------- shift-and-add (normalised convolution)
SHIFT_ADD_TILE = (8, 32)      # HRN_SHIFT_ADD_TILE_H x HRN_SHIFT_ADD_TILE_W: the LR pixels a workgroup of either kernel owns
SHIFT_ADD_MAX_SIDE = 16384    # hrn_shift_add: frames of 1 .. 16384 a side
SHIFT_ADD_SIGMA = (0.1, 1.0)  # the range of sigma, LR pixels


def shift_add(views, view_masks, alphas, shifts, base, scale, sigma, prior, want_weight=True, out=None):
    """hrn_shift_add on contiguous f32 device tensors (hrnet_hip/shiftadd.py checks them): views (B,V,H,W), view_masks the same or None,
    alphas (B,V) or None, shifts (B,V,2), base (B,SH,SW) or None -> (out (B,SH,SW), weight (B,SH,SW) or None).  out: where the result
    goes (a new tensor when None); base may be out itself."""
    lib = load_library()
    B, V, H, W = views.shape
    if out is None:
        out = torch.empty((B, scale * H, scale * W), dtype=torch.float32, device=views.device)
    weight = torch.empty((B, scale * H, scale * W), dtype=torch.float32, device=views.device) if want_weight else None
    with torch.cuda.device(views.device):
        _check(lib.hrn_shift_add(_ptr(views), _opt_ptr(view_masks), _opt_ptr(alphas), _ptr(shifts), _opt_ptr(base), _ptr(out), _opt_ptr(weight),
                                 B, V, H, W, int(scale), float(sigma), float(prior), _stream()), "hrn_shift_add")
    return out, weight


def shift_add_backward(d_out, weight, view_masks, alphas, shifts, V, H, W, scale, sigma, prior, need_views=True, need_base=True):
    """hrn_shift_add_backward: d_out, weight (B,SH,SW) contiguous f32 (weight: the forward's second result) -> (d_views (B,V,H,W) or None,
    d_base (B,SH,SW) or None), each computed only where needed; both unneeded is an error."""
    if not (need_views or need_base):
        raise ValueError("shift_add_backward: neither d_views nor d_base is asked for")
    lib = load_library()
    B = d_out.shape[0]
    d_views = torch.empty((B, V, H, W), dtype=torch.float32, device=d_out.device) if need_views else None
    d_base = torch.empty_like(d_out) if need_base else None
    with torch.cuda.device(d_out.device):
        _check(lib.hrn_shift_add_backward(_ptr(d_out), _ptr(weight), _opt_ptr(view_masks), _opt_ptr(alphas), _ptr(shifts), _opt_ptr(d_views),
                                          _opt_ptr(d_base), B, int(V), int(H), int(W), int(scale), float(sigma), float(prior), _stream()),
               "hrn_shift_add_backward")
    return d_views, d_base


# --------------------------------------------------------------------------- the observation model (observe.hip)
OBSERVE_TILE = (8, 32)        # HRN_OBSERVE_TILE_H x HRN_OBSERVE_TILE_W: the LR samples a workgroup owns
OBSERVE_MAX_SIDE = 16384      # frames of 1 .. 16384 a side
OBSERVE_STEP = (0.0, 2.0)     # back-projection's step lies strictly between these


def observe(hr, shifts, scale):
    """hrn_observe on contiguous f32 device tensors (hrnet_hip/observation.py checks them): hr (B,SH,SW), shifts (B,V,2) ->
    (views (B,V,H,W), valid (B,V,H,W) 0 / 1)."""
    lib = load_library()
    B, V = shifts.shape[:2]
    H, W = hr.shape[1] // scale, hr.shape[2] // scale
    views = torch.empty((B, V, H, W), dtype=torch.float32, device=hr.device)
    valid = torch.empty_like(views)
    with torch.cuda.device(hr.device):
        _check(lib.hrn_observe(_ptr(hr), _ptr(shifts), _ptr(views), _ptr(valid), B, V, H, W, int(scale), _stream()), "hrn_observe")
    return views, valid


def observe_adjoint(residual, lr_masks, alphas, shifts, beta, coef, gain, x, scale, out=None):
    """hrn_observe_adjoint: residual (B,V,H,W), beta (B,V) or None, coef, gain (B,) or None, x (B,SH,SW) or None -> out (B,SH,SW) =
    coef gain G, or x - coef gain G.  out: where the result goes (a new tensor when None); x may be out itself."""
    lib = load_library()
    B, V, H, W = residual.shape
    if out is None:
        out = torch.empty((B, scale * H, scale * W), dtype=torch.float32, device=residual.device)
    with torch.cuda.device(residual.device):
        _check(lib.hrn_observe_adjoint(_ptr(residual), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _opt_ptr(beta), _opt_ptr(coef),
                                       _opt_ptr(gain), _opt_ptr(x), _ptr(out), B, V, H, W, int(scale), _stream()), "hrn_observe_adjoint")
    return out


class ConsistencyState:
    """What the residual / finish pair of launches writes, allocated once and reused by every iteration of a back-projection: residual
    (B,V,H,W), the tiles' workspace, beta (B,V), count (B,V) int32, ssr (B,V) fp64, n_views (B,) int32, coef_loss, coef_step (B,)."""

    def __init__(self, B, V, H, W, device):
        lib = load_library()
        self.shape = (B, V, H, W)
        self.ws_bytes = int(lib.hrn_observe_workspace_bytes(B, V, H, W))
        if self.ws_bytes == 0:
            raise HrnetHipError(f"hrn_observe_workspace_bytes refuses B={B} V={V} H={H} W={W}")
        f32 = dict(dtype=torch.float32, device=device)
        self.workspace = torch.empty((self.ws_bytes // 8,), dtype=torch.float64, device=device)
        self.residual = torch.empty((B, V, H, W), **f32)
        self.beta = torch.empty((B, V), **f32)
        self.count = torch.empty((B, V), dtype=torch.int32, device=device)
        self.ssr = torch.empty((B, V), dtype=torch.float64, device=device)
        self.n_views = torch.empty((B,), dtype=torch.int32, device=device)
        self.coef_loss = torch.empty((B,), **f32)
        self.coef_step = torch.empty((B,), **f32)


def consistency_residual(hr, lrs, lr_masks, alphas, shifts, scale, step, brightness, state, loss):
    """hrn_consistency_residual then hrn_consistency_finish into `state` (a ConsistencyState) and `loss` (B,) f32: two launches, nothing
    returns to the host."""
    lib = load_library()
    B, V, H, W = state.shape
    with torch.cuda.device(hr.device):
        _check(lib.hrn_consistency_residual(_ptr(hr), _ptr(lrs), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _ptr(state.residual),
                                            _ptr(state.workspace), state.ws_bytes, B, V, H, W, int(scale), _stream()), "hrn_consistency_residual")
        _check(lib.hrn_consistency_finish(_ptr(state.workspace), state.ws_bytes, _ptr(state.beta), _ptr(state.count), _ptr(state.ssr), _ptr(loss),
                                          _ptr(state.n_views), _ptr(state.coef_loss), _ptr(state.coef_step), B, V, H, W, int(scale), float(step),
                                          int(bool(brightness)), _stream()), "hrn_consistency_finish")


def back_project(sr0, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness):
    """iters back-projection steps from sr0 (B,SH,SW): three launches each (residual, finish, adjoint in place) on the current stream ->
    (sr, losses (iters,B) = L_b of the frame each step STARTED from).  iters = 0 returns a copy of sr0."""
    B, V, H, W = lrs.shape
    x = sr0.clone()
    losses = torch.empty((iters, B), dtype=torch.float32, device=sr0.device)
    if iters:
        state = ConsistencyState(B, V, H, W, sr0.device)
        for t in range(iters):
            consistency_residual(x, lrs, lr_masks, alphas, shifts, scale, step, brightness, state, losses[t])
            observe_adjoint(state.residual, lr_masks, alphas, shifts, state.beta, state.coef_step, None, x, scale, out=x)
    return x, losses


# --------------------------------------------------------------------------- the derivative in the shifts (observe_shift.hip)
SHIFT_NORMAL_SUMS = 10        # HRN_SHIFT_NORMAL_SUMS: the doubles a tile leaves in the workspace
SHIFT_MIN_WEIGHT = 3.0        # a view whose sum p is below this keeps its shift


def shift_workspace(B, V, H, W, device):
    nbytes = int(load_library().hrn_observe_shift_workspace_bytes(B, V, H, W))
    if nbytes == 0:
        raise HrnetHipError(f"hrn_observe_shift_workspace_bytes refuses B={B} V={V} H={H} W={W}")
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device)


def observe_shift_grad(hr, g, lr_masks, alphas, shifts, beta, coef, gain, scale, workspace=None):
    """hrn_observe_shift_grad then hrn_observe_shift_grad_finish: hr (B,SH,SW), g (B,V,H,W), beta (B,V) or None, coef, gain (B,) or None ->
    d_shifts (B,V,2) = coef gain sum [counted] (g + beta) D.  Two launches."""
    lib = load_library()
    B, V, H, W = g.shape
    ws = shift_workspace(B, V, H, W, hr.device) if workspace is None else workspace
    out = torch.empty((B, V, 2), dtype=torch.float32, device=hr.device)
    with torch.cuda.device(hr.device):
        _check(lib.hrn_observe_shift_grad(_ptr(hr), _ptr(g), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _opt_ptr(beta), _ptr(ws),
                                          ws.numel() * 8, B, V, H, W, int(scale), _stream()), "hrn_observe_shift_grad")
        _check(lib.hrn_observe_shift_grad_finish(_ptr(ws), ws.numel() * 8, _opt_ptr(coef), _opt_ptr(gain), _ptr(out), B, V, H, W, _stream()),
               "hrn_observe_shift_grad_finish")
    return out


def shift_normal(hr, lrs, lr_masks, alphas, shifts, scale, brightness, beta_prev=None, delta=0.1, fixed=None, damping=0.0, max_step=1.0,
                 shifts_out=None, residual=None, workspace=None, normal=None, state=None, step=1.0, loss=None):
    """hrn_shift_normal then hrn_shift_normal_finish -> normal (B,V,8) fp64.  beta_prev (B,V): Welsch weights.  shifts_out (B,V,2): the
    damped Gauss-Newton update is written there (fixed: (B,V) uint8 or None).  residual (B,V,H,W): the residual plane too.  Two launches.
    state (a ConsistencyState) with loss (B,): the pass stands in for consistency_residual - it writes state.residual and the three plain
    sums into state.workspace, and hrn_consistency_finish runs on them between the two launches (three launches; the bits are
    consistency_residual's)."""
    lib = load_library()
    B, V, H, W = lrs.shape
    ws = shift_workspace(B, V, H, W, hr.device) if workspace is None else workspace
    if normal is None:
        normal = torch.empty((B, V, 8), dtype=torch.float64, device=hr.device)
    with torch.cuda.device(hr.device):
        if state is not None:
            residual = state.residual
        _check(lib.hrn_shift_normal(_ptr(hr), _ptr(lrs), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _opt_ptr(beta_prev), float(delta),
                                    _opt_ptr(residual), _opt_ptr(None if state is None else state.workspace), 0 if state is None else state.ws_bytes,
                                    _ptr(ws), ws.numel() * 8, B, V, H, W, int(scale), _stream()), "hrn_shift_normal")
        if state is not None:
            _check(lib.hrn_consistency_finish(_ptr(state.workspace), state.ws_bytes, _ptr(state.beta), _ptr(state.count), _ptr(state.ssr),
                                              _ptr(loss), _ptr(state.n_views), _ptr(state.coef_loss), _ptr(state.coef_step), B, V, H, W, int(scale),
                                              float(step), int(bool(brightness)), _stream()), "hrn_consistency_finish")
        _check(lib.hrn_shift_normal_finish(_ptr(ws), ws.numel() * 8, _opt_ptr(alphas), _ptr(shifts), _opt_ptr(fixed), _ptr(normal),
                                           _opt_ptr(shifts_out), B, V, H, W, int(scale), int(bool(brightness)), float(damping), float(max_step),
                                           _stream()), "hrn_shift_normal_finish")
    return normal


def refine_shifts(sr, lrs, lr_masks, alphas, shifts, fixed, scale, iters, damping, max_step, brightness, robust, delta):
    """iters Gauss-Newton steps on the shifts with the frame held, two launches each between two shift buffers -> (shifts', trace
    (iters,B,V,8): the normal equations every step started from).  robust: Welsch weights around the plain mean bias of each step's frame
    (hrn_consistency_residual + finish: two more launches a step)."""
    B, V, H, W = lrs.shape
    dev = sr.device
    cur, nxt = shifts.clone(), torch.empty_like(shifts)
    trace = torch.empty((iters, B, V, 8), dtype=torch.float64, device=dev)
    if iters:
        ws = shift_workspace(B, V, H, W, dev)
        state = ConsistencyState(B, V, H, W, dev) if robust else None
        loss = torch.empty((B,), dtype=torch.float32, device=dev) if robust else None
        for t in range(iters):
            if robust:
                consistency_residual(sr, lrs, lr_masks, alphas, cur, scale, 1.0, brightness, state, loss)
            shift_normal(sr, lrs, lr_masks, alphas, cur, scale, brightness, state.beta if robust else None, delta, fixed, damping, max_step,
                         shifts_out=nxt, workspace=ws, normal=trace[t])
            cur, nxt = nxt, cur
    return cur, trace


def reconstruct_joint(sr0, lrs, lr_masks, alphas, shifts, fixed, scale, iters, refine_every, refine_from, damping, max_step, step, brightness,
                      robust, delta, lam, P, alpha, eps):
    """`reconstruct`'s iteration (its launches, unchanged) with a shift update beside the data step of iteration t when refine_every > 0,
    t >= refine_from and (t - refine_from) % refine_every == 0 (with `robust` also t >= 1: the update's weights need a beta_prev).  The
    update reads the frame and the shifts the iteration started from and writes a second shift buffer, so the adjoint still runs on the
    old shifts; the buffers are swapped after the iteration.  In an updating iteration hrn_shift_normal takes the place of
    hrn_consistency_residual (one pass over the frame; hrn_consistency_finish runs on the plain sums it leaves) and
    hrn_shift_normal_finish is the one launch more -> (sr, shifts)."""
    B, V, H, W = lrs.shape
    dev = sr0.device
    x = sr0.clone()
    cur, nxt = shifts.clone(), torch.empty_like(shifts)
    if iters:
        state = ConsistencyState(B, V, H, W, dev)
        rstate = RobustState(B, V, H, W, dev) if robust else None
        loss, wloss = (torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(2))
        if refine_every > 0:
            ws = shift_workspace(B, V, H, W, dev)
            normal = torch.empty((B, V, 8), dtype=torch.float64, device=dev)
        if lam > 0:
            y = torch.empty_like(x)
            c = torch.full((B,), float(step) * float(lam), dtype=torch.float32, device=dev)
        for t in range(iters):
            refine = refine_every > 0 and t >= refine_from and (t - refine_from) % refine_every == 0 and not (robust and t == 0)
            if refine:                                   # the normal pass stands in for the residual pass: the same residual, sums and finish
                shift_normal(x, lrs, lr_masks, alphas, cur, scale, brightness, rstate.beta_prev if robust else None, delta, fixed, damping,
                             max_step, shifts_out=nxt, workspace=ws, normal=normal, state=state, step=step, loss=loss)
            else:
                consistency_residual(x, lrs, lr_masks, alphas, cur, scale, step, brightness, state, loss)
            if robust and t == 0:
                rstate.beta_prev.copy_(state.beta)
            if robust:
                robust_step(state, rstate, lr_masks, alphas, cur, scale, delta, brightness, wloss)
                observe_adjoint(rstate.weighted, lr_masks, alphas, cur, None, state.coef_step, None, x, scale, out=x)
                rstate.beta_prev, rstate.beta = rstate.beta, rstate.beta_prev
            else:
                observe_adjoint(state.residual, lr_masks, alphas, cur, state.beta, state.coef_step, None, x, scale, out=x)
            if lam > 0:
                btv_step(x, c, P, alpha, eps, out=y)
                x, y = y, x
            if refine:
                cur, nxt = nxt, cur
    return x, cur


# --------------------------------------------------------------------------- robust, regularised reconstruction (robust_sr.hip)
BTV_TILE = (16, 64)           # HRN_BTV_TILE_H x HRN_BTV_TILE_W: the HR pixels a workgroup owns
BTV_MAX_P = 3                 # the window's radius is 1 .. 3
BTV_MAX_SIDE = 49152          # planes of 1 .. 3 x 16384 a side
DATA_EIGENVALUE = 1.02        # the bound on the data operator's largest eigenvalue


def btv_weight_sum(P, alpha):
    """W = sum over (l, m) != (0, 0), |l|, |m| <= P, of alpha^(|l| + |m|)"""
    return sum(float(alpha) ** (abs(l) + abs(m)) for l in range(-P, P + 1) for m in range(-P, P + 1) if (l, m) != (0, 0))


def step_bound(step, lam, P, alpha, eps):
    """step (1.02 + 4 lam W / eps): the iteration of `reconstruct` is stable while this is below 2"""
    return float(step) * (DATA_EIGENVALUE + 4.0 * float(lam) * btv_weight_sum(P, alpha) / float(eps))


def btv_step(x, c, P, alpha, eps, out):
    """hrn_btv_step: x (planes,SH,SW), c (planes,) -> out = x - c g(x); out is another tensor than x."""
    lib = load_library()
    n, SH, SW = x.shape
    with torch.cuda.device(x.device):
        _check(lib.hrn_btv_step(_ptr(x), _ptr(c), _ptr(out), n, SH, SW, int(P), float(alpha), float(eps), _stream()), "hrn_btv_step")
    return out


def btv_backward(x, gain, P, alpha, eps):
    """hrn_btv_backward: x (planes,SH,SW), gain (planes,) -> gain g(x), a new tensor."""
    lib = load_library()
    n, SH, SW = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _check(lib.hrn_btv_backward(_ptr(x), _ptr(gain), _ptr(out), n, SH, SW, int(P), float(alpha), float(eps), _stream()), "hrn_btv_backward")
    return out


def btv_workspace(n, SH, SW, device):
    nbytes = int(load_library().hrn_btv_workspace_bytes(n, SH, SW))
    if nbytes == 0:
        raise HrnetHipError(f"hrn_btv_workspace_bytes refuses planes={n} SH={SH} SW={SW}")
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device)


def btv_value(x, P, alpha, eps, gain=1.0, out=None, workspace=None):
    """hrn_btv_value: x (planes,SH,SW) -> (planes,) f32 = gain R(x) / (SH SW).  out, workspace: reused when given."""
    lib = load_library()
    n, SH, SW = x.shape
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = btv_workspace(n, SH, SW, x.device)
    with torch.cuda.device(x.device):
        _check(lib.hrn_btv_value(_ptr(x), _ptr(out), _ptr(workspace), workspace.numel() * 8, n, SH, SW, int(P), float(alpha), float(eps),
                                 float(gain), _stream()), "hrn_btv_value")
    return out


class RobustState:
    """What the robust data step writes, allocated once per reconstruction: the tiles' workspace, beta_prev and beta (B,V) (swapped after
    every iteration), the inlier fraction (B,V) and the re-weighted residual (B,V,H,W) that the adjoint reads."""

    def __init__(self, B, V, H, W, device):
        lib = load_library()
        self.shape = (B, V, H, W)
        self.ws_bytes = int(lib.hrn_robust_workspace_bytes(B, V, H, W))
        if self.ws_bytes == 0:
            raise HrnetHipError(f"hrn_robust_workspace_bytes refuses B={B} V={V} H={H} W={W}")
        f32 = dict(dtype=torch.float32, device=device)
        self.workspace = torch.empty((self.ws_bytes // 8,), dtype=torch.float64, device=device)
        self.beta_prev = torch.empty((B, V), **f32)
        self.beta = torch.empty((B, V), **f32)
        self.inlier = torch.empty((B, V), **f32)
        self.weighted = torch.empty((B, V, H, W), **f32)


def robust_step(cstate, rstate, lr_masks, alphas, shifts, scale, delta, brightness, loss):
    """hrn_robust_sums, hrn_robust_finish and hrn_robust_apply on the residual in `cstate` (a ConsistencyState that consistency_residual
    has filled): rstate.beta, .inlier, .weighted and `loss` (B,) are written; rstate.beta_prev is read."""
    lib = load_library()
    B, V, H, W = rstate.shape
    with torch.cuda.device(shifts.device):
        _check(lib.hrn_robust_sums(_ptr(cstate.residual), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _ptr(rstate.beta_prev),
                                   _ptr(rstate.workspace), rstate.ws_bytes, B, V, H, W, int(scale), float(delta), _stream()), "hrn_robust_sums")
        _check(lib.hrn_robust_finish(_ptr(rstate.workspace), rstate.ws_bytes, _ptr(cstate.count), _ptr(rstate.beta), _ptr(rstate.inlier),
                                     _ptr(loss), B, V, H, W, int(bool(brightness)), _stream()), "hrn_robust_finish")
        _check(lib.hrn_robust_apply(_ptr(cstate.residual), _opt_ptr(lr_masks), _opt_ptr(alphas), _ptr(shifts), _ptr(rstate.beta_prev),
                                    _ptr(rstate.beta), _ptr(rstate.weighted), B, V, H, W, int(scale), float(delta), _stream()),
               "hrn_robust_apply")


def reconstruct(sr0, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness, robust, delta, lam, P, alpha, eps, want_trace=True):
    """iters iterations from sr0 (B,SH,SW) on the current stream, nothing returning to the host: the data step - back_project's three
    launches, or with `robust` residual, finish, the three robust launches and the adjoint of the re-weighted residual - and with lam > 0
    the bilateral-TV half-step between two frames -> (sr, trace (iters,B,3)): the plain consistency loss, the weighted loss (the plain one
    again without `robust`) and lam R / pixels (0 without the prior, or when want_trace is off) of the frame each iteration STARTED from."""
    B, V, H, W = lrs.shape
    dev = sr0.device
    x = sr0.clone()
    plain, weighted, prior = (torch.zeros((iters, B), dtype=torch.float32, device=dev) for _ in range(3))
    if iters:
        state = ConsistencyState(B, V, H, W, dev)
        rstate = RobustState(B, V, H, W, dev) if robust else None
        if lam > 0:
            y = torch.empty_like(x)
            c = torch.full((B,), float(step) * float(lam), dtype=torch.float32, device=dev)
            ws = btv_workspace(B, x.shape[1], x.shape[2], dev) if want_trace else None
        for t in range(iters):
            if lam > 0 and want_trace:
                btv_value(x, P, alpha, eps, gain=lam, out=prior[t], workspace=ws)
            consistency_residual(x, lrs, lr_masks, alphas, shifts, scale, step, brightness, state, plain[t])
            if robust:
                if t == 0:
                    rstate.beta_prev.copy_(state.beta)
                robust_step(state, rstate, lr_masks, alphas, shifts, scale, delta, brightness, weighted[t])
                observe_adjoint(rstate.weighted, lr_masks, alphas, shifts, None, state.coef_step, None, x, scale, out=x)
                rstate.beta_prev, rstate.beta = rstate.beta, rstate.beta_prev
            else:
                observe_adjoint(state.residual, lr_masks, alphas, shifts, state.beta, state.coef_step, None, x, scale, out=x)
            if lam > 0:
                btv_step(x, c, P, alpha, eps, out=y)
                x, y = y, x
        if not robust:
            weighted = plain.clone()
    return x, torch.stack((plain, weighted, prior), dim=2)


# --------------------------------------------------------------------------- PyTorch-ROCm custom ops (north_star: "exposed to Python as
# PyTorch-ROCm custom ops"): the inference entry points are registered with the dispatcher as torch.ops.hrnet_hip.*, with fake
# (meta) implementations, so that they are visible to torch.compile / export and to anyone calling through torch.ops.  Each is a
# thin shim over the ctypes call above - the C ABI stays the boundary.  The reference-named modules call THESE in eval mode.
@torch.library.custom_op("hrnet_hip::hrnet_forward", mutates_args=(), device_types="cuda")
def _op_hrnet_forward(packed: torch.Tensor, dtype: int, num_layers: int, alpha_residual: bool, lrs: torch.Tensor,
                      alphas: torch.Tensor, scale: int = 3) -> torch.Tensor:
    return hrnet_forward(packed, dtype, num_layers, alpha_residual, lrs, alphas, scale=scale)


@_op_hrnet_forward.register_fake
def _(packed, dtype, num_layers, alpha_residual, lrs, alphas, scale=3):
    b, _, h, w = lrs.shape
    return lrs.new_empty((b, 1, scale * h, scale * w), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::hrnet_forward_ref", mutates_args=(), device_types="cuda")
def _op_hrnet_forward_ref(packed: torch.Tensor, dtype: int, num_layers: int, alpha_residual: bool, lrs: torch.Tensor,
                          alphas: torch.Tensor, ref: torch.Tensor, scale: int = 3) -> torch.Tensor:
    """hrnet_forward with the reference frame `ref` (B,H,W) in place of the median of lrs[:, :9] (hrn_hrnet_forward_ref)."""
    return hrnet_forward(packed, dtype, num_layers, alpha_residual, lrs, alphas, scale=scale, ref=ref)


@_op_hrnet_forward_ref.register_fake
def _(packed, dtype, num_layers, alpha_residual, lrs, alphas, ref, scale=3):
    b, _, h, w = lrs.shape
    return lrs.new_empty((b, 1, scale * h, scale * w), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::masked_composite", mutates_args=(), device_types="cuda")
def _op_masked_composite(lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor], n_ref: int, want_count: bool,
                         fill: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """hrn_masked_composite: (ref (B,H,W), filled (B,V,H,W), count (B,H,W)); an output that was not asked for comes back empty.  No
    gradient: the frame is data."""
    ref, filled, count = masked_composite(lrs, lr_masks, alphas, n_ref, want_count, fill)
    return (ref, filled if fill else lrs.new_empty((0,), dtype=torch.float32),
            count if want_count else lrs.new_empty((0,), dtype=torch.float32))


@_op_masked_composite.register_fake
def _(lrs, lr_masks, alphas, n_ref, want_count, fill):
    b, _, h, w = lrs.shape
    return (lrs.new_empty((b, h, w), dtype=torch.float32), lrs.new_empty(lrs.shape if fill else (0,), dtype=torch.float32),
            lrs.new_empty((b, h, w) if want_count else (0,), dtype=torch.float32))


# Bicubic upsampling with an add (upsample.hip): out = base + up(frames).  Linear in both inputs: d_frames is the adjoint kernel applied
# to d_out (a registered op itself), d_base is d_out.
@torch.library.custom_op("hrnet_hip::upsample", mutates_args=(), device_types="cuda")
def _op_upsample(frames: torch.Tensor, base: Optional[torch.Tensor], scale: int, a: float) -> torch.Tensor:
    """frames (N,H,W), base (N,scale H,scale W) or None -> base + up(frames), f32 (hrn_upsample)."""
    return upsample(frames.float().contiguous(), None if base is None else base.float().contiguous(), scale, a)


@_op_upsample.register_fake
def _(frames, base, scale, a):
    n, h, w = frames.shape
    return frames.new_empty((n, scale * h, scale * w), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::upsample_backward", mutates_args=(), device_types="cuda")
def _op_upsample_backward(d_out: torch.Tensor, H: int, W: int, scale: int, a: float) -> torch.Tensor:
    """d_out (N,scale H,scale W) -> d_frames (N,H,W), the adjoint of up() (hrn_upsample_backward)."""
    return upsample_backward(d_out.float().contiguous(), H, W, scale, a)


@_op_upsample_backward.register_fake
def _(d_out, H, W, scale, a):
    return d_out.new_empty((d_out.shape[0], H, W), dtype=torch.float32)


def _upsample_setup(ctx, inputs, output):
    frames, base, scale, a = inputs
    ctx.hw, ctx.scale, ctx.a = tuple(frames.shape[1:]), scale, a
    ctx.frames_dtype, ctx.base_dtype = frames.dtype, None if base is None else base.dtype


def _upsample_backward(ctx, d_out):
    need_frames, need_base = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    d_frames = torch.ops.hrnet_hip.upsample_backward(d_out, ctx.hw[0], ctx.hw[1], ctx.scale, ctx.a).to(ctx.frames_dtype) if need_frames else None
    return d_frames, (d_out.to(ctx.base_dtype) if need_base else None), None, None


_op_upsample.register_autograd(_upsample_backward, setup_context=_upsample_setup)


# Shift-and-add (shift_add.hip): (out, weight) = hrn_shift_add.  out is linear in views and base; weight depends on masks and shifts only
# and carries no gradient, nor do shifts, masks and alphas.  The autograd formula is hrn_shift_add_backward (a registered op itself) on
# the saved weight.
def _f32c(t):
    return None if t is None else t.float().contiguous()


@torch.library.custom_op("hrnet_hip::shift_add", mutates_args=(), device_types="cuda")
def _op_shift_add(views: torch.Tensor, view_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor], shifts: torch.Tensor,
                  base: Optional[torch.Tensor], scale: int, sigma: float, prior: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """views (B,V,H,W), view_masks or None, alphas (B,V) or None, shifts (B,V,2), base (B,SH,SW) or None -> (out, weight) (hrn_shift_add)."""
    return shift_add(_f32c(views), _f32c(view_masks), _f32c(alphas), _f32c(shifts), _f32c(base), scale, sigma, prior)


@_op_shift_add.register_fake
def _(views, view_masks, alphas, shifts, base, scale, sigma, prior):
    b, _, h, w = views.shape
    return (views.new_empty((b, scale * h, scale * w), dtype=torch.float32), views.new_empty((b, scale * h, scale * w), dtype=torch.float32))


@torch.library.custom_op("hrnet_hip::shift_add_backward", mutates_args=(), device_types="cuda")
def _op_shift_add_backward(d_out: torch.Tensor, weight: torch.Tensor, view_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                           shifts: torch.Tensor, V: int, H: int, W: int, scale: int, sigma: float, prior: float, need_views: bool,
                           need_base: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (d_views (B,V,H,W), d_base (B,SH,SW)) (hrn_shift_add_backward); a half that is not needed is an empty tensor and does not run."""
    d_views, d_base = shift_add_backward(_f32c(d_out), _f32c(weight), _f32c(view_masks), _f32c(alphas), _f32c(shifts), V, H, W, scale, sigma,
                                         prior, need_views, need_base)
    empty = d_out.new_empty((0,), dtype=torch.float32)
    return (empty if d_views is None else d_views), (empty.clone() if d_base is None else d_base)


@_op_shift_add_backward.register_fake
def _(d_out, weight, view_masks, alphas, shifts, V, H, W, scale, sigma, prior, need_views, need_base):
    b = d_out.shape[0]
    return (d_out.new_empty((b, V, H, W) if need_views else (0,), dtype=torch.float32),
            d_out.new_empty(tuple(d_out.shape) if need_base else (0,), dtype=torch.float32))


def _shift_add_setup(ctx, inputs, output):
    views, view_masks, alphas, shifts, base, scale, sigma, prior = inputs
    ctx.vhw, ctx.scale, ctx.sigma, ctx.prior = tuple(views.shape[1:]), scale, sigma, prior
    ctx.views_dtype, ctx.base_dtype = views.dtype, None if base is None else base.dtype
    ctx.has = (view_masks is not None, alphas is not None)
    ctx.save_for_backward(output[1], shifts, *(t for t in (view_masks, alphas) if t is not None))


def _shift_add_backward(ctx, d_out, d_weight):
    need_views, need_base = ctx.needs_input_grad[0], ctx.needs_input_grad[4]
    if not (need_views or need_base):
        return (None,) * 8
    saved = list(ctx.saved_tensors)
    weight, shifts = saved[0], saved[1]
    rest = saved[2:]
    view_masks = rest.pop(0) if ctx.has[0] else None
    alphas = rest.pop(0) if ctx.has[1] else None
    V, H, W = ctx.vhw
    d_views, d_base = torch.ops.hrnet_hip.shift_add_backward(d_out, weight, view_masks, alphas, shifts, V, H, W, ctx.scale, ctx.sigma,
                                                             ctx.prior, need_views, need_base)
    return (d_views.to(ctx.views_dtype) if need_views else None, None, None, None, d_base.to(ctx.base_dtype) if need_base else None,
            None, None, None)


_op_shift_add.register_autograd(_shift_add_backward, setup_context=_shift_add_setup)


# The observation model (observe.hip).  observe is linear in hr: its autograd formula is the adjoint of the incoming gradient (a
# registered op itself).  consistency_loss_train returns the loss with what its backward needs (the residual plane, beta, 2 / sum n); the
# formula is consistency_loss_backward.  There is no gradient to lrs, shifts, masks or alphas.  back_project carries no gradient at all.
@torch.library.custom_op("hrnet_hip::observe", mutates_args=(), device_types="cuda")
def _op_observe(hr: torch.Tensor, shifts: torch.Tensor, scale: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """hr (B,SH,SW), shifts (B,V,2) -> (views (B,V,H,W), valid (B,V,H,W) 0 / 1) (hrn_observe)."""
    return observe(_f32c(hr), _f32c(shifts), scale)


@_op_observe.register_fake
def _(hr, shifts, scale):
    shape = (hr.shape[0], shifts.shape[1], hr.shape[1] // scale, hr.shape[2] // scale)
    return hr.new_empty(shape, dtype=torch.float32), hr.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::observe_backward", mutates_args=(), device_types="cuda")
def _op_observe_backward(d_views: torch.Tensor, shifts: torch.Tensor, scale: int) -> torch.Tensor:
    """d_views (B,V,H,W) -> d_hr (B,SH,SW) = sum_v A_v^T [valid] d_views (hrn_observe_adjoint)."""
    return observe_adjoint(_f32c(d_views), None, None, _f32c(shifts), None, None, None, None, scale)


@_op_observe_backward.register_fake
def _(d_views, shifts, scale):
    b, _, h, w = d_views.shape
    return d_views.new_empty((b, scale * h, scale * w), dtype=torch.float32)


def _observe_setup(ctx, inputs, output):
    hr, shifts, scale = inputs
    ctx.scale, ctx.hr_dtype = scale, hr.dtype
    ctx.save_for_backward(shifts)


def _observe_backward(ctx, d_views, d_valid):
    if not ctx.needs_input_grad[0]:
        return None, None, None
    (shifts,) = ctx.saved_tensors
    return torch.ops.hrnet_hip.observe_backward(d_views, shifts, ctx.scale).to(ctx.hr_dtype), None, None


_op_observe.register_autograd(_observe_backward, setup_context=_observe_setup)


@torch.library.custom_op("hrnet_hip::consistency_loss_train", mutates_args=(), device_types="cuda")
def _op_consistency_loss_train(srs: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                               shifts: torch.Tensor, scale: int, brightness: bool
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """srs (B,SH,SW), lrs (B,V,H,W) -> (loss (B,), residual (B,V,H,W), beta (B,V), count (B,V) int32, coef (B,) = 2 / sum n)."""
    srs, lrs = _f32c(srs), _f32c(lrs)
    B, V, H, W = lrs.shape
    state = ConsistencyState(B, V, H, W, srs.device)
    loss = torch.empty((B,), dtype=torch.float32, device=srs.device)
    consistency_residual(srs, lrs, _f32c(lr_masks), _f32c(alphas), _f32c(shifts), scale, 1.0, brightness, state, loss)
    return loss, state.residual, state.beta, state.count, state.coef_loss


@_op_consistency_loss_train.register_fake
def _(srs, lrs, lr_masks, alphas, shifts, scale, brightness):
    b, v = lrs.shape[:2]
    f32 = dict(dtype=torch.float32)
    return (srs.new_empty((b,), **f32), srs.new_empty(tuple(lrs.shape), **f32), srs.new_empty((b, v), **f32),
            srs.new_empty((b, v), dtype=torch.int32), srs.new_empty((b,), **f32))


@torch.library.custom_op("hrnet_hip::consistency_loss_backward", mutates_args=(), device_types="cuda")
def _op_consistency_loss_backward(d_loss: torch.Tensor, residual: torch.Tensor, beta: torch.Tensor, coef: torch.Tensor,
                                  lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor], shifts: torch.Tensor,
                                  scale: int) -> torch.Tensor:
    """-> d_srs (B,SH,SW) = d_loss_b coef_b sum_v A_v^T r_v (hrn_observe_adjoint)."""
    return observe_adjoint(_f32c(residual), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), _f32c(beta), _f32c(coef), _f32c(d_loss), None, scale)


@_op_consistency_loss_backward.register_fake
def _(d_loss, residual, beta, coef, lr_masks, alphas, shifts, scale):
    b, _, h, w = residual.shape
    return residual.new_empty((b, scale * h, scale * w), dtype=torch.float32)


def _consistency_setup(ctx, inputs, output):
    srs, lrs, lr_masks, alphas, shifts, scale, brightness = inputs
    ctx.scale, ctx.srs_dtype = scale, srs.dtype
    ctx.has = (lr_masks is not None, alphas is not None)
    ctx.save_for_backward(output[1], output[2], output[4], shifts, *(t for t in (lr_masks, alphas) if t is not None))


def _consistency_backward(ctx, d_loss, d_residual, d_beta, d_count, d_coef):
    if not ctx.needs_input_grad[0]:
        return (None,) * 7
    saved = list(ctx.saved_tensors)
    residual, beta, coef, shifts = saved[:4]
    rest = saved[4:]
    lr_masks = rest.pop(0) if ctx.has[0] else None
    alphas = rest.pop(0) if ctx.has[1] else None
    d_srs = torch.ops.hrnet_hip.consistency_loss_backward(d_loss, residual, beta, coef, lr_masks, alphas, shifts, ctx.scale)
    return (d_srs.to(ctx.srs_dtype),) + (None,) * 6


_op_consistency_loss_train.register_autograd(_consistency_backward, setup_context=_consistency_setup)


@torch.library.custom_op("hrnet_hip::back_project", mutates_args=(), device_types="cuda")
def _op_back_project(sr0: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                     shifts: torch.Tensor, scale: int, iters: int, step: float, brightness: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sr (B,SH,SW) after `iters` back-projection steps from sr0, losses (iters,B)); no gradient."""
    return back_project(_f32c(sr0), _f32c(lrs), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), scale, iters, step, brightness)


@_op_back_project.register_fake
def _(sr0, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness):
    return sr0.new_empty(tuple(sr0.shape), dtype=torch.float32), sr0.new_empty((iters, sr0.shape[0]), dtype=torch.float32)


# The derivative in the shifts (observe_shift.hip).  observe_sg and consistency_loss_sg are observe and consistency_loss_train - the same
# launches, the same bits - whose autograd formulas also return d_shifts (observe_shift_backward), each half only when it is asked for.
# shift_normal, refine_shifts and reconstruct_joint carry no gradient.
@torch.library.custom_op("hrnet_hip::observe_shift_backward", mutates_args=(), device_types="cuda")
def _op_observe_shift_backward(hr: torch.Tensor, g: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                               shifts: torch.Tensor, beta: Optional[torch.Tensor], coef: Optional[torch.Tensor],
                               gain: Optional[torch.Tensor], scale: int) -> torch.Tensor:
    """-> d_shifts (B,V,2) = coef gain sum [counted] (g + beta) D (hrn_observe_shift_grad, hrn_observe_shift_grad_finish)."""
    return observe_shift_grad(_f32c(hr), _f32c(g), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), _f32c(beta), _f32c(coef), _f32c(gain), scale)


@_op_observe_shift_backward.register_fake
def _(hr, g, lr_masks, alphas, shifts, beta, coef, gain, scale):
    return hr.new_empty(tuple(shifts.shape), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::observe_sg", mutates_args=(), device_types="cuda")
def _op_observe_sg(hr: torch.Tensor, shifts: torch.Tensor, scale: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """observe, differentiable in hr and in shifts."""
    return observe(_f32c(hr), _f32c(shifts), scale)


@_op_observe_sg.register_fake
def _(hr, shifts, scale):
    shape = (hr.shape[0], shifts.shape[1], hr.shape[1] // scale, hr.shape[2] // scale)
    return hr.new_empty(shape, dtype=torch.float32), hr.new_empty(shape, dtype=torch.float32)


def _observe_sg_setup(ctx, inputs, output):
    hr, shifts, scale = inputs
    ctx.scale, ctx.hr_dtype, ctx.shifts_dtype = scale, hr.dtype, shifts.dtype
    ctx.save_for_backward(hr, shifts)


def _observe_sg_backward(ctx, d_views, d_valid):
    hr, shifts = ctx.saved_tensors
    d_hr = d_shifts = None
    if ctx.needs_input_grad[0]:
        d_hr = torch.ops.hrnet_hip.observe_backward(d_views, shifts, ctx.scale).to(ctx.hr_dtype)
    if ctx.needs_input_grad[1]:
        d_shifts = torch.ops.hrnet_hip.observe_shift_backward(hr, d_views, None, None, shifts, None, None, None, ctx.scale).to(ctx.shifts_dtype)
    return d_hr, d_shifts, None


_op_observe_sg.register_autograd(_observe_sg_backward, setup_context=_observe_sg_setup)


@torch.library.custom_op("hrnet_hip::consistency_loss_sg", mutates_args=(), device_types="cuda")
def _op_consistency_loss_sg(srs: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                            shifts: torch.Tensor, scale: int, brightness: bool
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """consistency_loss_train, differentiable in srs and in shifts."""
    srs, lrs = _f32c(srs), _f32c(lrs)
    B, V, H, W = lrs.shape
    state = ConsistencyState(B, V, H, W, srs.device)
    loss = torch.empty((B,), dtype=torch.float32, device=srs.device)
    consistency_residual(srs, lrs, _f32c(lr_masks), _f32c(alphas), _f32c(shifts), scale, 1.0, brightness, state, loss)
    return loss, state.residual, state.beta, state.count, state.coef_loss


@_op_consistency_loss_sg.register_fake
def _(srs, lrs, lr_masks, alphas, shifts, scale, brightness):
    b, v = lrs.shape[:2]
    f32 = dict(dtype=torch.float32)
    return (srs.new_empty((b,), **f32), srs.new_empty(tuple(lrs.shape), **f32), srs.new_empty((b, v), **f32),
            srs.new_empty((b, v), dtype=torch.int32), srs.new_empty((b,), **f32))


def _consistency_sg_setup(ctx, inputs, output):
    srs, lrs, lr_masks, alphas, shifts, scale, brightness = inputs
    ctx.scale, ctx.srs_dtype, ctx.shifts_dtype = scale, srs.dtype, shifts.dtype
    ctx.has = (lr_masks is not None, alphas is not None)
    ctx.save_for_backward(output[1], output[2], output[4], shifts, srs, *(t for t in (lr_masks, alphas) if t is not None))


def _consistency_sg_backward(ctx, d_loss, d_residual, d_beta, d_count, d_coef):
    saved = list(ctx.saved_tensors)
    residual, beta, coef, shifts, srs = saved[:5]
    rest = saved[5:]
    lr_masks = rest.pop(0) if ctx.has[0] else None
    alphas = rest.pop(0) if ctx.has[1] else None
    d_srs = d_shifts = None
    if ctx.needs_input_grad[0]:
        d_srs = torch.ops.hrnet_hip.consistency_loss_backward(d_loss, residual, beta, coef, lr_masks, alphas, shifts, ctx.scale).to(ctx.srs_dtype)
    if ctx.needs_input_grad[4]:
        d_shifts = torch.ops.hrnet_hip.observe_shift_backward(srs, residual, lr_masks, alphas, shifts, beta, coef, d_loss,
                                                              ctx.scale).to(ctx.shifts_dtype)
    return d_srs, None, None, None, d_shifts, None, None


_op_consistency_loss_sg.register_autograd(_consistency_sg_backward, setup_context=_consistency_sg_setup)


@torch.library.custom_op("hrnet_hip::shift_normal", mutates_args=(), device_types="cuda")
def _op_shift_normal(sr: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                     shifts: torch.Tensor, beta_prev: Optional[torch.Tensor], scale: int, brightness: bool, delta: float) -> torch.Tensor:
    """-> normal (B,V,8) fp64 (hrn_shift_normal, hrn_shift_normal_finish); beta_prev: Welsch weights; no gradient."""
    return shift_normal(_f32c(sr), _f32c(lrs), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), scale, brightness, _f32c(beta_prev), delta)


@_op_shift_normal.register_fake
def _(sr, lrs, lr_masks, alphas, shifts, beta_prev, scale, brightness, delta):
    return sr.new_empty((lrs.shape[0], lrs.shape[1], 8), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::refine_shifts", mutates_args=(), device_types="cuda")
def _op_refine_shifts(sr: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                      shifts: torch.Tensor, fixed: Optional[torch.Tensor], scale: int, iters: int, damping: float, max_step: float,
                      brightness: bool, robust: bool, delta: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (shifts' (B,V,2), trace (iters,B,V,8) fp64); fixed (B,V) uint8 or None; no gradient."""
    return refine_shifts(_f32c(sr), _f32c(lrs), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), fixed, scale, iters, damping, max_step,
                         brightness, robust, delta)


@_op_refine_shifts.register_fake
def _(sr, lrs, lr_masks, alphas, shifts, fixed, scale, iters, damping, max_step, brightness, robust, delta):
    return (sr.new_empty(tuple(shifts.shape), dtype=torch.float32), sr.new_empty((iters,) + tuple(shifts.shape[:2]) + (8,), dtype=torch.float64))


@torch.library.custom_op("hrnet_hip::reconstruct_joint", mutates_args=(), device_types="cuda")
def _op_reconstruct_joint(sr0: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                          shifts: torch.Tensor, fixed: Optional[torch.Tensor], scale: int, iters: int, refine_every: int, refine_from: int,
                          damping: float, max_step: float, step: float, brightness: bool, robust: bool, delta: float, lam: float, P: int,
                          alpha: float, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sr (B,SH,SW), shifts (B,V,2)) after `iters` iterations of reconstruct with shift updates; no gradient."""
    return reconstruct_joint(_f32c(sr0), _f32c(lrs), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), fixed, scale, iters, refine_every,
                             refine_from, damping, max_step, step, brightness, robust, delta, lam, P, alpha, eps)


@_op_reconstruct_joint.register_fake
def _(sr0, lrs, lr_masks, alphas, shifts, fixed, scale, iters, refine_every, refine_from, damping, max_step, step, brightness, robust, delta,
      lam, P, alpha, eps):
    return sr0.new_empty(tuple(sr0.shape), dtype=torch.float32), sr0.new_empty(tuple(shifts.shape), dtype=torch.float32)


# Robust, regularised reconstruction (robust_sr.hip).  reconstruct carries no gradient.  btv_loss_train is R / pixels per plane; its
# autograd formula is btv_loss_backward, the same kernel as the half-step with out = gain g.
@torch.library.custom_op("hrnet_hip::reconstruct", mutates_args=(), device_types="cuda")
def _op_reconstruct(sr0: torch.Tensor, lrs: torch.Tensor, lr_masks: Optional[torch.Tensor], alphas: Optional[torch.Tensor],
                    shifts: torch.Tensor, scale: int, iters: int, step: float, brightness: bool, robust: bool, delta: float, lam: float,
                    P: int, alpha: float, eps: float, trace: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sr (B,SH,SW) after `iters` iterations from sr0, trace (iters,B,3)); robust: Welsch weights; no gradient."""
    return reconstruct(_f32c(sr0), _f32c(lrs), _f32c(lr_masks), _f32c(alphas), _f32c(shifts), scale, iters, step, brightness, robust, delta, lam,
                       P, alpha, eps, trace)


@_op_reconstruct.register_fake
def _(sr0, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness, robust, delta, lam, P, alpha, eps, trace):
    return sr0.new_empty(tuple(sr0.shape), dtype=torch.float32), sr0.new_empty((iters, sr0.shape[0], 3), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::btv_loss_train", mutates_args=(), device_types="cuda")
def _op_btv_loss_train(srs: torch.Tensor, P: int, alpha: float, eps: float) -> torch.Tensor:
    """srs (B,SH,SW) -> (B,) = R(srs_b) / (SH SW) (hrn_btv_value)."""
    return btv_value(_f32c(srs), P, alpha, eps)


@_op_btv_loss_train.register_fake
def _(srs, P, alpha, eps):
    return srs.new_empty((srs.shape[0],), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::btv_loss_backward", mutates_args=(), device_types="cuda")
def _op_btv_loss_backward(d_loss: torch.Tensor, srs: torch.Tensor, P: int, alpha: float, eps: float) -> torch.Tensor:
    """-> d_srs (B,SH,SW) = (d_loss_b / (SH SW)) g(srs_b) (hrn_btv_backward)."""
    srs = _f32c(srs)
    gain = (_f32c(d_loss) / float(srs.shape[1] * srs.shape[2])).contiguous()
    return btv_backward(srs, gain, P, alpha, eps)


@_op_btv_loss_backward.register_fake
def _(d_loss, srs, P, alpha, eps):
    return srs.new_empty(tuple(srs.shape), dtype=torch.float32)


def _btv_setup(ctx, inputs, output):
    srs, ctx.P, ctx.alpha, ctx.eps = inputs
    ctx.srs_dtype = srs.dtype
    ctx.save_for_backward(srs)


def _btv_backward(ctx, d_loss):
    if not ctx.needs_input_grad[0]:
        return None, None, None, None
    (srs,) = ctx.saved_tensors
    return torch.ops.hrnet_hip.btv_loss_backward(d_loss, srs, ctx.P, ctx.alpha, ctx.eps).to(ctx.srs_dtype), None, None, None


_op_btv_loss_train.register_autograd(_btv_backward, setup_context=_btv_setup)


@torch.library.custom_op("hrnet_hip::lanczos_shift", mutates_args=(), device_types="cuda")
def _op_lanczos_shift(img: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    return lanczos_shift(img, shift)


@_op_lanczos_shift.register_fake
def _(img, shift):
    return img.new_empty(img.shape, dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::lanczos_kernel", mutates_args=(), device_types="cuda")
def _op_lanczos_kernel(dx: torch.Tensor) -> torch.Tensor:
    return lanczos_kernel(dx)


@_op_lanczos_kernel.register_fake
def _(dx):
    return dx.new_empty((dx.numel(), 7), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::shift_cpsnr", mutates_args=(), device_types="cuda")
def _op_shift_cpsnr(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, border_w: int, clip: bool) -> torch.Tensor:
    return shift_cpsnr(srs, hrs, hr_maps, border_w, clip)


@_op_shift_cpsnr.register_fake
def _(srs, hrs, hr_maps, border_w, clip):
    return srs.new_empty((srs.shape[0] if srs.dim() == 3 else 1,), dtype=torch.float32)


# the two ends of the self-ensemble (HRNet.forward_ensemble): inference only, so no autograd formula
@torch.library.custom_op("hrnet_hip::dihedral_expand", mutates_args=(), device_types="cuda")
def _op_dihedral_expand(x: torch.Tensor, codes: Sequence[int]) -> torch.Tensor:
    return dihedral_expand(x, codes)


@_op_dihedral_expand.register_fake
def _(x, codes):
    return x.new_empty((len(codes),) + tuple(x.shape), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::dihedral_mean", mutates_args=(), device_types="cuda")
def _op_dihedral_mean(y: torch.Tensor, codes: Sequence[int]) -> torch.Tensor:
    return dihedral_mean(y, codes)


@_op_dihedral_mean.register_fake
def _(y, codes):
    return y.new_empty(tuple(y.shape[1:]), dtype=torch.float32)


# the two ends of tiled inference (HRNet.forward_tiled): inference only, so no autograd formula
@torch.library.custom_op("hrnet_hip::tile_gather", mutates_args=(), device_types="cuda")
def _op_tile_gather(lrs: torch.Tensor, t: int, R: int, w0: int, w1: int) -> torch.Tensor:
    return tile_gather(lrs, t, R, w0, w1)


@_op_tile_gather.register_fake
def _(lrs, t, R, w0, w1):
    return lrs.new_empty((w1 - w0,) + tuple(lrs.shape[:2]) + (t, t), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::tile_scatter", mutates_args=("out",), device_types="cuda")
def _op_tile_scatter(out: torch.Tensor, srs: torch.Tensor, t: int, R: int, scale: int, w0: int, w1: int) -> None:
    tile_scatter(out, srs, t, R, scale, w0, w1)


# --------------------------------------------------------------------------- the TRAINING entry points as dispatcher-registered ops
# (call sites: src/train.py:174-191).  Each is registered with a fake (meta) implementation and, where the reference differentiates
# through it, with `register_autograd`: the backward formula is itself a registered op over the C ABI's *_backward entry point.  The
# reference-named modules call these through torch.ops.hrnet_hip.* in .train() mode.
SHIFTNET_PARAM_NAMES = [f"layer{i}.{j}.{k}" for i in range(1, 9) for j in (0, 1) for k in ("weight", "bias")] + ["fc1.weight", "fc1.bias", "fc2.weight"]
SHIFTNET_BUFFER_NAMES = [f"layer{i}.1.{k}" for i in range(1, 9) for k in ("running_mean", "running_var")]


@torch.library.custom_op("hrnet_hip::hrnet_forward_train", mutates_args=(), device_types="cuda")
def _op_hrnet_forward_train(packed: torch.Tensor, lrs: torch.Tensor, alphas: torch.Tensor, params: Sequence[torch.Tensor],
                            num_layers: int, alpha_residual: bool, dtype: int, scale: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """`srs = fusion_model(lrs, alphas)` in training (train.py:174): the forward that keeps every intermediate in `tws`, in fp32 (dtype 0),
    bf16 (dtype 1) or split-bf16 (dtype 2).  `packed` is the blob of `params` for that dtype (the raw parameters travel along for the backward pass and
    as the differentiable inputs).  `scale`: the upscale factor the blob was packed for; sr is (B, 1, scale H, scale W)."""
    return hrnet_forward_train(packed, lrs, alphas, num_layers, alpha_residual, dtype, scale)


@_op_hrnet_forward_train.register_fake
def _(packed, lrs, alphas, params, num_layers, alpha_residual, dtype, scale=3):
    b, v, h, w = lrs.shape
    nbytes = load_library().hrn_hrnet_train_workspace_bytes(num_layers, b, v, h, w)
    return lrs.new_empty((b, 1, scale * h, scale * w), dtype=torch.float32), lrs.new_empty((nbytes,), dtype=torch.uint8)


def _hrnet_backward_body(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, need_params=None,
                         need_lrs=False, need_alphas=False, ref=None, need_ref=False):
    """The three HRNet backward ops: (parameter gradients in `hrnet_param_names` order, d_lrs, d_alphas), an empty tensor for whatever
    was not asked for.  need_params None: every parameter; else need_params[i] says whether params[i] wants a gradient."""
    names = hrnet_param_names(num_layers)
    if need_params is not None and len(need_params) != len(names):
        raise ValueError(f"need_params has {len(need_params)} entries for {len(names)} parameters")
    named = dict(zip(names, params))
    grads = {k: torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
             for i, (k, p) in enumerate(named.items()) if need_params is None or need_params[i]}
    d_lrs = torch.empty(lrs.shape, dtype=torch.float32, device=lrs.device) if need_lrs else None
    d_alphas = torch.empty(alphas.shape, dtype=torch.float32, device=alphas.device) if need_alphas else None
    if ref is not None:
        d_ref = torch.empty(ref.shape, dtype=torch.float32, device=ref.device) if need_ref else None
        hrnet_backward(packed, named, grads, num_layers, alpha_residual, lrs, alphas, d_sr.contiguous(), tws, dtype, scale, d_lrs=d_lrs,
                       d_alphas=d_alphas, select=True, ref=ref, d_ref=d_ref)
        return ([grads[k] if k in grads else named[k].new_empty((0,), dtype=torch.float32) for k in names],
                d_lrs if need_lrs else lrs.new_empty((0,), dtype=torch.float32),
                d_alphas if need_alphas else alphas.new_empty((0,), dtype=torch.float32),
                d_ref if need_ref else ref.new_empty((0,), dtype=torch.float32))
    hrnet_backward(packed, named, grads, num_layers, alpha_residual, lrs, alphas, d_sr.contiguous(), tws, dtype, scale, d_lrs=d_lrs,
                   d_alphas=d_alphas, select=need_params is not None)
    return ([grads[k] if k in grads else named[k].new_empty((0,), dtype=torch.float32) for k in names],
            d_lrs if need_lrs else lrs.new_empty((0,), dtype=torch.float32),
            d_alphas if need_alphas else alphas.new_empty((0,), dtype=torch.float32))


@torch.library.custom_op("hrnet_hip::hrnet_backward", mutates_args=("tws",), device_types="cuda")     # (tws also holds the backward's scratch buffers)
def _op_hrnet_backward(packed: torch.Tensor, params: Sequence[torch.Tensor], lrs: torch.Tensor, alphas: torch.Tensor, d_sr: torch.Tensor,
                       tws: torch.Tensor, num_layers: int, alpha_residual: bool, dtype: int, scale: int = 3) -> List[torch.Tensor]:
    """d_sr -> the gradient of every parameter (train.py:190 through HRNet), in `hrnet_param_names` order."""
    return _hrnet_backward_body(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale)[0]


@_op_hrnet_backward.register_fake
def _(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale=3):
    return [p.new_empty(p.shape, dtype=torch.float32) for p in params]


@torch.library.custom_op("hrnet_hip::hrnet_backward_in", mutates_args=("tws",), device_types="cuda")
def _op_hrnet_backward_in(packed: torch.Tensor, params: Sequence[torch.Tensor], lrs: torch.Tensor, alphas: torch.Tensor, d_sr: torch.Tensor,
                          tws: torch.Tensor, num_layers: int, alpha_residual: bool, dtype: int, scale: int, need_lrs: bool,
                          need_alphas: bool) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """hrnet_backward that also returns the input gradients (HRNet.py:198-204, :113-132): (parameter gradients in `hrnet_param_names`
    order, d_lrs (B,V,H,W), d_alphas (B,V)); an input gradient that was not asked for comes back empty."""
    return _hrnet_backward_body(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, None, need_lrs, need_alphas)


@_op_hrnet_backward_in.register_fake
def _(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, need_lrs, need_alphas):
    return ([p.new_empty(p.shape, dtype=torch.float32) for p in params],
            lrs.new_empty(lrs.shape if need_lrs else (0,), dtype=torch.float32),
            alphas.new_empty(alphas.shape if need_alphas else (0,), dtype=torch.float32))


@torch.library.custom_op("hrnet_hip::hrnet_backward_sel", mutates_args=("tws",), device_types="cuda")
def _op_hrnet_backward_sel(packed: torch.Tensor, params: Sequence[torch.Tensor], lrs: torch.Tensor, alphas: torch.Tensor, d_sr: torch.Tensor,
                           tws: torch.Tensor, num_layers: int, alpha_residual: bool, dtype: int, scale: int, need_params: Sequence[bool],
                           need_lrs: bool, need_alphas: bool) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """hrnet_backward_in for a partly frozen model (hrn_hrnet_backward_sel): need_params[i] says whether params[i] wants a gradient.
    Returns (parameter gradients in `hrnet_param_names` order, an empty tensor for every frozen one; d_lrs; d_alphas); only the work the
    requested outputs depend on is launched, and each of them is bit-identical to hrnet_backward_in's."""
    return _hrnet_backward_body(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, list(need_params), need_lrs,
                                need_alphas)


@_op_hrnet_backward_sel.register_fake
def _(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, need_params, need_lrs, need_alphas):
    return ([p.new_empty(p.shape if need else (0,), dtype=torch.float32) for p, need in zip(params, need_params)],
            lrs.new_empty(lrs.shape if need_lrs else (0,), dtype=torch.float32),
            alphas.new_empty(alphas.shape if need_alphas else (0,), dtype=torch.float32))


def _hrnet_train_setup(ctx, inputs, output):
    packed, lrs, alphas, params, num_layers, alpha_residual, dtype, scale = inputs
    ctx.num_layers, ctx.alpha_residual, ctx.n, ctx.dtype, ctx.scale = num_layers, alpha_residual, len(params), dtype, scale
    # which parameters autograd will ask for (requires_grad_(False): frozen)
    ctx.need_params = [bool(p.requires_grad) for p in params]
    ctx.set_materialize_grads(False)          # (or autograd hands the backward a zero-filled "gradient" of the 20 GB workspace output)
    ctx.save_for_backward(packed, lrs, alphas, output[1], *params)


def _hrnet_train_backward(ctx, d_sr, _d_tws):
    packed, lrs, alphas, tws, *params = ctx.saved_tensors
    # one entry per input as the caller passed them: a trailing `scale` equal to its default is not among them
    tail = (None,) * (len(ctx.needs_input_grad) - 4)
    if d_sr is None:
        return (None, None, None, [None] * len(params)) + tail
    # (tws.data: the backward's scratch buffers live in tws too, so the op declares it mutated; through an alias with its own version
    # counter the saved tensor stays valid for a second backward pass - backward(retain_graph=True), the kept intermediates are only read)
    # input gradients only when autograd asks for them; alphas reach the reference's graph only through the alpha residual of a
    # fusion level (HRNet.py:124-128), so without one (or with a single view) their gradient stays None, as in the reference
    need_lrs = ctx.needs_input_grad[1]
    need_alphas = ctx.needs_input_grad[2] and bool(ctx.alpha_residual) and lrs.shape[1] > 1
    if not (any(ctx.need_params) or need_lrs or need_alphas):
        return (None, None, None, [None] * len(params)) + tail
    # frozen parameters get None (their .grad stays None) and their work is not launched
    grads, d_lrs, d_alphas = torch.ops.hrnet_hip.hrnet_backward_sel(packed, params, lrs, alphas, d_sr, tws.data, ctx.num_layers,
                                                                    ctx.alpha_residual, ctx.dtype, ctx.scale, ctx.need_params,
                                                                    need_lrs, need_alphas)
    return (None, d_lrs.to(lrs.dtype) if need_lrs else None, d_alphas.to(alphas.dtype) if need_alphas else None,
            [g.to(p.dtype) if need else None for g, p, need in zip(grads, params, ctx.need_params)]) + tail


_op_hrnet_forward_train.register_autograd(_hrnet_train_backward, setup_context=_hrnet_train_setup)


# the training pair with the reference frame given (hrn_hrnet_forward_train_ref / hrn_hrnet_backward_ref)
@torch.library.custom_op("hrnet_hip::hrnet_forward_train_ref", mutates_args=(), device_types="cuda")
def _op_hrnet_forward_train_ref(packed: torch.Tensor, lrs: torch.Tensor, alphas: torch.Tensor, ref: torch.Tensor,
                                params: Sequence[torch.Tensor], num_layers: int, alpha_residual: bool, dtype: int,
                                scale: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """hrnet_forward_train with the reference frame `ref` (B,H,W) contiguous f32 in place of the median of lrs[:, :9]; `ref` is a
    differentiable input of its own (its gradient: the stem's second input channel summed over the views)."""
    return hrnet_forward_train(packed, lrs, alphas, num_layers, alpha_residual, dtype, scale, ref=ref)


@_op_hrnet_forward_train_ref.register_fake
def _(packed, lrs, alphas, ref, params, num_layers, alpha_residual, dtype, scale=3):
    b, v, h, w = lrs.shape
    nbytes = load_library().hrn_hrnet_train_workspace_bytes(num_layers, b, v, h, w)
    return lrs.new_empty((b, 1, scale * h, scale * w), dtype=torch.float32), lrs.new_empty((nbytes,), dtype=torch.uint8)


@torch.library.custom_op("hrnet_hip::hrnet_backward_ref", mutates_args=("tws",), device_types="cuda")
def _op_hrnet_backward_ref(packed: torch.Tensor, params: Sequence[torch.Tensor], lrs: torch.Tensor, alphas: torch.Tensor, ref: torch.Tensor,
                           d_sr: torch.Tensor, tws: torch.Tensor, num_layers: int, alpha_residual: bool, dtype: int, scale: int,
                           need_params: Sequence[bool], need_lrs: bool, need_alphas: bool,
                           need_ref: bool) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor, torch.Tensor]:
    """hrnet_backward_sel for a forward that was given its reference frame (hrn_hrnet_backward_ref): (parameter gradients, d_lrs - the
    stem's channel 0 alone -, d_alphas, d_ref (B,H,W)); whatever was not asked for comes back empty."""
    return _hrnet_backward_body(packed, params, lrs, alphas, d_sr, tws, num_layers, alpha_residual, dtype, scale, list(need_params), need_lrs,
                                need_alphas, ref=ref, need_ref=need_ref)


@_op_hrnet_backward_ref.register_fake
def _(packed, params, lrs, alphas, ref, d_sr, tws, num_layers, alpha_residual, dtype, scale, need_params, need_lrs, need_alphas, need_ref):
    return ([p.new_empty(p.shape if need else (0,), dtype=torch.float32) for p, need in zip(params, need_params)],
            lrs.new_empty(lrs.shape if need_lrs else (0,), dtype=torch.float32),
            alphas.new_empty(alphas.shape if need_alphas else (0,), dtype=torch.float32),
            ref.new_empty(ref.shape if need_ref else (0,), dtype=torch.float32))


def _hrnet_train_ref_setup(ctx, inputs, output):
    packed, lrs, alphas, ref, params, num_layers, alpha_residual, dtype, scale = inputs
    ctx.num_layers, ctx.alpha_residual, ctx.n, ctx.dtype, ctx.scale = num_layers, alpha_residual, len(params), dtype, scale
    ctx.need_params = [bool(p.requires_grad) for p in params]
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(packed, lrs, alphas, ref, output[1], *params)


def _hrnet_train_ref_backward(ctx, d_sr, _d_tws):
    packed, lrs, alphas, ref, tws, *params = ctx.saved_tensors
    tail = (None,) * (len(ctx.needs_input_grad) - 5)
    none = (None, None, None, None, [None] * len(params)) + tail
    if d_sr is None:
        return none
    need_lrs, need_ref = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
    need_alphas = ctx.needs_input_grad[2] and bool(ctx.alpha_residual) and lrs.shape[1] > 1
    if not (any(ctx.need_params) or need_lrs or need_alphas or need_ref):
        return none
    grads, d_lrs, d_alphas, d_ref = torch.ops.hrnet_hip.hrnet_backward_ref(packed, params, lrs, alphas, ref, d_sr, tws.data, ctx.num_layers,
                                                                           ctx.alpha_residual, ctx.dtype, ctx.scale, ctx.need_params,
                                                                           need_lrs, need_alphas, need_ref)
    return (None, d_lrs.to(lrs.dtype) if need_lrs else None, d_alphas.to(alphas.dtype) if need_alphas else None,
            d_ref.to(ref.dtype) if need_ref else None,
            [g.to(p.dtype) if need else None for g, p, need in zip(grads, params, ctx.need_params)]) + tail


_op_hrnet_forward_train_ref.register_autograd(_hrnet_train_ref_backward, setup_context=_hrnet_train_ref_setup)


def _shiftnet_named(params, buffers):
    named = dict(zip(SHIFTNET_PARAM_NAMES, params))
    named.update(zip(SHIFTNET_BUFFER_NAMES, buffers))
    return named


@torch.library.custom_op("hrnet_hip::shiftnet_forward_train", mutates_args=(), device_types="cuda")
def _op_shiftnet_forward_train(packed: torch.Tensor, x: torch.Tensor, params: Sequence[torch.Tensor], bn_running: Sequence[torch.Tensor],
                               momentum: float, dropout_mask: Optional[torch.Tensor],
                               dtype: int = 0) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
    """`shifts = regis_model(pairs)` in training (train.py:40): batch-statistics BatchNorm, the given dropout keep-mask; keeps each layer's
    pre-BatchNorm tensor and statistics in `tws` for the backward.  Functional (an op with an autograd formula must be): the updated
    running statistics come back as new tensors, in SHIFTNET_BUFFER_NAMES order, and the module copies them into its buffers.  dtype:
    the storage of the kept activations and gradients, fp32 (0, the default) or bf16 (1); `packed` is the fp32 blob in both."""
    new_running = [b.clone() for b in bn_running]
    theta, tws = shiftnet_forward_train(packed, _shiftnet_named(params, new_running), x, momentum=momentum, dropout_mask=dropout_mask,
                                        dtype=dtype)
    return theta, tws, new_running


@_op_shiftnet_forward_train.register_fake
def _(packed, x, params, bn_running, momentum, dropout_mask, dtype=0):
    nbytes = load_library().hrn_shiftnet_train_workspace_bytes_dt(dtype, x.shape[0])
    return x.new_empty((x.shape[0], 2), dtype=torch.float32), x.new_empty((nbytes,), dtype=torch.uint8), [b.new_empty(b.shape) for b in bn_running]


def _shiftnet_backward_body(params, x, dropout_mask, d_theta, tws, need_input_grad, dtype, need_params=None):
    """The two ShiftNet backward ops: (parameter gradients in SHIFTNET_PARAM_NAMES order, an empty tensor for every frozen one; d_x, empty
    when not needed).  need_params None: every parameter.  The batch statistics the backward needs are in `tws`; the running statistics
    take no part (the BatchNorm weights stand in for them in the C struct)."""
    if need_params is not None and len(need_params) != len(SHIFTNET_PARAM_NAMES):
        raise ValueError(f"need_params has {len(need_params)} entries for {len(SHIFTNET_PARAM_NAMES)} parameters")
    named = dict(zip(SHIFTNET_PARAM_NAMES, params))
    for k in SHIFTNET_BUFFER_NAMES:
        named[k] = named[k.rsplit(".", 1)[0] + ".weight"]
    grads = {k: torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
             for i, (k, p) in enumerate(zip(SHIFTNET_PARAM_NAMES, params)) if need_params is None or need_params[i]}
    d_x = shiftnet_backward(named, grads, x, dropout_mask, d_theta.contiguous(), tws, need_input_grad=need_input_grad, dtype=dtype,
                            select=need_params is not None)
    return ([grads[k] if k in grads else named[k].new_empty((0,), dtype=torch.float32) for k in SHIFTNET_PARAM_NAMES],
            (d_x if d_x is not None else x.new_empty((0,))))


@torch.library.custom_op("hrnet_hip::shiftnet_backward", mutates_args=("tws",), device_types="cuda")  # (tws also holds the backward's scratch buffers)
def _op_shiftnet_backward(params: Sequence[torch.Tensor], x: torch.Tensor,
                          dropout_mask: Optional[torch.Tensor], d_theta: torch.Tensor, tws: torch.Tensor,
                          need_input_grad: bool, dtype: int = 0) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """d_theta -> (parameter gradients in SHIFTNET_PARAM_NAMES order, d_x (empty when not needed))."""
    return _shiftnet_backward_body(params, x, dropout_mask, d_theta, tws, need_input_grad, dtype)


@_op_shiftnet_backward.register_fake
def _(params, x, dropout_mask, d_theta, tws, need_input_grad, dtype=0):
    return [p.new_empty(p.shape, dtype=torch.float32) for p in params], (x.new_empty(x.shape) if need_input_grad else x.new_empty((0,)))


@torch.library.custom_op("hrnet_hip::shiftnet_backward_sel", mutates_args=("tws",), device_types="cuda")
def _op_shiftnet_backward_sel(params: Sequence[torch.Tensor], x: torch.Tensor, dropout_mask: Optional[torch.Tensor], d_theta: torch.Tensor,
                              tws: torch.Tensor, need_input_grad: bool, dtype: int,
                              need_params: Sequence[bool]) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """shiftnet_backward for a partly frozen ShiftNet (hrn_shiftnet_backward_sel): need_params[i] says whether params[i] wants a gradient.
    Returns (parameter gradients in SHIFTNET_PARAM_NAMES order, an empty tensor for every frozen one; d_x, empty when not needed)."""
    return _shiftnet_backward_body(params, x, dropout_mask, d_theta, tws, need_input_grad, dtype, list(need_params))


@_op_shiftnet_backward_sel.register_fake
def _(params, x, dropout_mask, d_theta, tws, need_input_grad, dtype, need_params):
    return ([p.new_empty(p.shape if need else (0,), dtype=torch.float32) for p, need in zip(params, need_params)],
            (x.new_empty(x.shape) if need_input_grad else x.new_empty((0,))))


def _shiftnet_train_setup(ctx, inputs, output):
    packed, x, params, bn_running, momentum, dropout_mask = inputs[:6]
    ctx.np, ctx.has_mask = len(params), dropout_mask is not None
    ctx.need_params = [bool(p.requires_grad) for p in params]          # as in _hrnet_train_setup
    ctx.dtype = inputs[6] if len(inputs) > 6 else F32
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(x, output[1], *params, *([dropout_mask] if dropout_mask is not None else []))


def _shiftnet_train_backward(ctx, d_theta, _d_tws, _d_running):
    x, tws, *rest = ctx.saved_tensors
    # one entry per input as the caller passed them: a trailing `dtype` equal to its default is not among them
    tail = (None,) * (len(ctx.needs_input_grad) - 4)
    if d_theta is None:
        return (None, None, [None] * ctx.np, [None] * len(SHIFTNET_BUFFER_NAMES)) + tail
    params = rest[:ctx.np]
    mask = rest[ctx.np] if ctx.has_mask else None
    need_x = ctx.needs_input_grad[1]
    # a wholly frozen ShiftNet (e.g. a fixed pretrained registration model) only passes d_x back into HRNet, or nothing at all
    if not (any(ctx.need_params) or need_x):
        return (None, None, [None] * ctx.np, [None] * len(SHIFTNET_BUFFER_NAMES)) + tail
    grads, d_x = torch.ops.hrnet_hip.shiftnet_backward_sel(params, x, mask, d_theta, tws.data, need_x, ctx.dtype,      # (tws.data: see
                                                           ctx.need_params)                                           # _hrnet_train_backward)
    return (None, (d_x if need_x else None), [g if need else None for g, need in zip(grads, ctx.need_params)],
            [None] * len(SHIFTNET_BUFFER_NAMES)) + tail


_op_shiftnet_forward_train.register_autograd(_shiftnet_train_backward, setup_context=_shiftnet_train_setup)


@torch.library.custom_op("hrnet_hip::lanczos_shift_backward", mutates_args=(), device_types="cuda")
def _op_lanczos_shift_backward(img: torch.Tensor, shift: torch.Tensor, d_out: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Adjoint of lanczos_shift wrt the image and the gradient wrt the shifts (through the 7 taps per axis): (d_img, d_shift (c, 2))."""
    d_img, d_shift = lanczos_shift_backward(img, shift, d_out.contiguous(), True, True)
    full = torch.zeros_like(shift, dtype=torch.float32)
    full[:d_shift.shape[0]] = d_shift                       # `shift` may carry more rows than img has channels
    return d_img, full


@_op_lanczos_shift_backward.register_fake
def _(img, shift, d_out):
    return img.new_empty(img.shape, dtype=torch.float32), shift.new_empty(shift.shape, dtype=torch.float32)


def _lanczos_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.set_materialize_grads(False)


def _lanczos_backward(ctx, d_out):
    img, shift = ctx.saved_tensors
    if d_out is None:
        return None, None
    d_img, d_shift = torch.ops.hrnet_hip.lanczos_shift_backward(img, shift, d_out)
    return (d_img.to(img.dtype) if ctx.needs_input_grad[0] else None), (d_shift.to(shift.dtype) if ctx.needs_input_grad[1] else None)


_op_lanczos_shift.register_autograd(_lanczos_backward, setup_context=_lanczos_setup)


@torch.library.custom_op("hrnet_hip::get_loss_train", mutates_args=(), device_types="cuda")
def _op_get_loss_train(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, metric: str, crop: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The registered-loss tail (train.py:78-87, :183-187): (loss per sample (B,), stats (B,4) f64 = {n, bias, cMSE, 0})."""
    return get_loss_train(srs, hrs, hr_maps, metric, crop)


@_op_get_loss_train.register_fake
def _(srs, hrs, hr_maps, metric, crop):
    return srs.new_empty((srs.shape[0],), dtype=torch.float32), srs.new_empty((srs.shape[0], 4), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::get_loss_backward", mutates_args=(), device_types="cuda")
def _op_get_loss_backward(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, stats: torch.Tensor, d_out: torch.Tensor,
                          metric: str, crop: int) -> torch.Tensor:
    return get_loss_backward(srs, hrs, hr_maps, stats, d_out.contiguous(), metric, crop)


@_op_get_loss_backward.register_fake
def _(srs, hrs, hr_maps, stats, d_out, metric, crop):
    return srs.new_empty(srs.shape, dtype=torch.float32)


def _loss_setup(ctx, inputs, output):
    srs, hrs, hr_maps, ctx.metric, ctx.crop = inputs
    ctx.save_for_backward(srs, hrs, hr_maps, output[1])
    ctx.set_materialize_grads(False)


def _loss_backward(ctx, d_out, _d_stats):
    srs, hrs, hr_maps, stats = ctx.saved_tensors
    if d_out is None:
        return None, None, None, None, None
    return torch.ops.hrnet_hip.get_loss_backward(srs, hrs, hr_maps, stats, d_out, ctx.metric, ctx.crop), None, None, None, None


_op_get_loss_train.register_autograd(_loss_backward, setup_context=_loss_setup)


@torch.library.custom_op("hrnet_hip::shift_loss_train", mutates_args=(), device_types="cuda")
def _op_shift_loss_train(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, metric: str, border_w: int,
                         clip: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The shift-searched loss (Evaluator.py:52-73 over train.py:66-87): (loss per sample (B,), stats (B,4) f64 = {n, bias, cMSE, k})."""
    return shift_loss_train(srs, hrs, hr_maps, metric, border_w, clip)


@_op_shift_loss_train.register_fake
def _(srs, hrs, hr_maps, metric, border_w, clip):
    return srs.new_empty((srs.shape[0],), dtype=torch.float32), srs.new_empty((srs.shape[0], 4), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::shift_loss_backward", mutates_args=(), device_types="cuda")
def _op_shift_loss_backward(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, stats: torch.Tensor, d_out: torch.Tensor,
                            metric: str, border_w: int, clip: bool) -> torch.Tensor:
    return shift_loss_backward(srs, hrs, hr_maps, stats, d_out.contiguous(), metric, border_w, clip)


@_op_shift_loss_backward.register_fake
def _(srs, hrs, hr_maps, stats, d_out, metric, border_w, clip):
    return srs.new_empty(srs.shape, dtype=torch.float32)


def _register_searched_loss(train_op, backward_name, n_args):
    """The autograd of a searched loss: train_op(srs, hrs, hr_maps, *args) -> (out, stats), d_srs = the op hrnet_hip::<backward_name>
    (srs, hrs, hr_maps, stats, d_out, *args) of the same n_args non-tensor arguments; the targets and their status maps get no gradient."""
    def setup(ctx, inputs, output):
        ctx.args = tuple(inputs[3:])
        ctx.save_for_backward(*inputs[:3], output[1])
        ctx.set_materialize_grads(False)

    def backward(ctx, d_out, _d_stats):
        if d_out is None:
            return (None,) * (3 + n_args)
        return (getattr(torch.ops.hrnet_hip, backward_name)(*ctx.saved_tensors, d_out, *ctx.args),) + (None,) * (2 + n_args)

    train_op.register_autograd(backward, setup_context=setup)


_register_searched_loss(_op_shift_loss_train, "shift_loss_backward", 3)


# cSSIM is a score: no autograd formula.
@torch.library.custom_op("hrnet_hip::shift_cssim", mutates_args=(), device_types="cuda")
def _op_shift_cssim(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, border_w: int, window: str, clip: bool,
                    correct_bias: bool, data_range: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The shift-searched SSIM: (score per sample (B,), stats (B,4) f64 = {n, bias, score, k}, scores (B, (2 border_w + 1)^2) f64)."""
    return shift_cssim(srs, hrs, hr_maps, border_w, window, clip, correct_bias, data_range)


@_op_shift_cssim.register_fake
def _(srs, hrs, hr_maps, border_w, window, clip, correct_bias, data_range):
    B = srs.shape[0]
    return (srs.new_empty((B,), dtype=torch.float32), srs.new_empty((B, 4), dtype=torch.float64),
            srs.new_empty((B, (2 * border_w + 1) ** 2), dtype=torch.float64))


# cSSIM as a loss: the same forward without the per-offset scores, and the gradient through the selected offset.
@torch.library.custom_op("hrnet_hip::shift_cssim_train", mutates_args=(), device_types="cuda")
def _op_shift_cssim_train(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, border_w: int, window: str, clip: bool,
                          correct_bias: bool, data_range: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The shift-searched SSIM, differentiable in srs: (score per sample (B,), stats (B,4) f64 = {n, bias, score, k})."""
    return shift_cssim(srs, hrs, hr_maps, border_w, window, clip, correct_bias, data_range, with_scores=False)[:2]


@_op_shift_cssim_train.register_fake
def _(srs, hrs, hr_maps, border_w, window, clip, correct_bias, data_range):
    return srs.new_empty((srs.shape[0],), dtype=torch.float32), srs.new_empty((srs.shape[0], 4), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::cssim_loss_backward", mutates_args=(), device_types="cuda")
def _op_cssim_loss_backward(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, stats: torch.Tensor, d_out: torch.Tensor,
                            border_w: int, window: str, clip: bool, correct_bias: bool, data_range: float) -> torch.Tensor:
    return cssim_loss_backward(srs, hrs, hr_maps, stats, d_out.contiguous(), border_w, window, clip, correct_bias, data_range)


@_op_cssim_loss_backward.register_fake
def _(srs, hrs, hr_maps, stats, d_out, border_w, window, clip, correct_bias, data_range):
    return srs.new_empty(srs.shape, dtype=torch.float32)


_register_searched_loss(_op_shift_cssim_train, "cssim_loss_backward", 5)


# The shift-searched L1 / Charbonnier: the gradient through the selected offset, the bias attached.
@torch.library.custom_op("hrnet_hip::cl1_loss_train", mutates_args=(), device_types="cuda")
def _op_cl1_loss_train(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, border_w: int, clip: bool,
                       eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The shift-searched L1 / Charbonnier: (loss per sample (B,), stats (B,5) f64 = {n, bias, cL1, k, sigma})."""
    return cl1_loss_train(srs, hrs, hr_maps, border_w, clip, eps)


@_op_cl1_loss_train.register_fake
def _(srs, hrs, hr_maps, border_w, clip, eps):
    return srs.new_empty((srs.shape[0],), dtype=torch.float32), srs.new_empty((srs.shape[0], 5), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::cl1_loss_backward", mutates_args=(), device_types="cuda")
def _op_cl1_loss_backward(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, stats: torch.Tensor, d_out: torch.Tensor,
                          border_w: int, clip: bool, eps: float) -> torch.Tensor:
    return cl1_loss_backward(srs, hrs, hr_maps, stats, d_out.contiguous(), border_w, clip, eps)


@_op_cl1_loss_backward.register_fake
def _(srs, hrs, hr_maps, stats, d_out, border_w, clip, eps):
    return srs.new_empty(srs.shape, dtype=torch.float32)


_register_searched_loss(_op_cl1_loss_train, "cl1_loss_backward", 3)


# The sub-pixel searched cMSE / cPSNR: the gradient through the sampler at the point the search found, which is held fixed.
@torch.library.custom_op("hrnet_hip::subpixel_loss_train", mutates_args=(), device_types="cuda")
def _op_subpixel_loss_train(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, metric: str, border_w: int, points_per_dim: int,
                            levels: int, radius: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The sub-pixel searched loss: (loss per sample (B,), stats (B,8) f64 = {n*, b*, cMSE*, dy*, dx*, mean sr, mean hr, centred bias},
    trace (B,levels,3) f32)."""
    return subpixel_loss_train(srs, hrs, hr_maps, metric, border_w, points_per_dim, levels, radius)


@_op_subpixel_loss_train.register_fake
def _(srs, hrs, hr_maps, metric, border_w, points_per_dim, levels, radius):
    B = srs.shape[0]
    return (srs.new_empty((B,), dtype=torch.float32), srs.new_empty((B, SUBPIXEL_STATS), dtype=torch.float64),
            srs.new_empty((B, levels, 3), dtype=torch.float32))


@torch.library.custom_op("hrnet_hip::subpixel_loss_backward", mutates_args=(), device_types="cuda")
def _op_subpixel_loss_backward(srs: torch.Tensor, hrs: torch.Tensor, hr_maps: torch.Tensor, stats: torch.Tensor, d_out: torch.Tensor,
                               metric: str, border_w: int) -> torch.Tensor:
    return subpixel_loss_backward(srs, hrs, hr_maps, stats, d_out.contiguous(), metric, border_w)


@_op_subpixel_loss_backward.register_fake
def _(srs, hrs, hr_maps, stats, d_out, metric, border_w):
    return srs.new_empty(srs.shape, dtype=torch.float32)


def _subpixel_setup(ctx, inputs, output):
    ctx.metric, ctx.border_w = inputs[3], inputs[4]
    ctx.save_for_backward(*inputs[:3], output[1])
    ctx.set_materialize_grads(False)


def _subpixel_backward(ctx, d_out, _d_stats, _d_trace):
    if d_out is None or not ctx.needs_input_grad[0]:      # stats and trace carry no gradient; no launch unless srs needs one
        return (None,) * 8
    return (torch.ops.hrnet_hip.subpixel_loss_backward(*ctx.saved_tensors, d_out, ctx.metric, ctx.border_w),) + (None,) * 7


_op_subpixel_loss_train.register_autograd(_subpixel_backward, setup_context=_subpixel_setup)


# The registration search has no autograd formula: a shift found by a grid search is piecewise constant in the frames.
@torch.library.custom_op("hrnet_hip::mncc_grid", mutates_args=(), device_types="cuda")
def _op_mncc_grid(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                  centres: torch.Tensor, points_per_dim: int, width: float) -> torch.Tensor:
    return mncc_grid(ref, ref_mask, views, view_masks, centres, points_per_dim, width)


@_op_mncc_grid.register_fake
def _fake_mncc_grid(ref, ref_mask, views, view_masks, centres, points_per_dim, width):
    return views.new_empty((views.shape[0], views.shape[1], points_per_dim, points_per_dim), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::mncc_search", mutates_args=(), device_types="cuda")
def _op_mncc_search(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                    points_per_dim: int, levels: int, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_search(ref, ref_mask, views, view_masks, points_per_dim, levels, radius)


@_op_mncc_search.register_fake
def _fake_mncc_search(ref, ref_mask, views, view_masks, points_per_dim, levels, radius):
    B, V = views.shape[:2]
    return views.new_empty((B, V, 2), dtype=torch.float32), views.new_empty((B, V, levels, 3), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::shift_views", mutates_args=(), device_types="cuda")
def _op_shift_views(views: torch.Tensor, view_masks: Optional[torch.Tensor], shifts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_apply(views, view_masks, shifts)


@_op_shift_views.register_fake
def _fake_shift_views(views, view_masks, shifts):
    return views.new_empty(views.shape, dtype=torch.float32), views.new_empty(views.shape, dtype=torch.float32)


# the same three for frames of any size (registration_scene.hip)
@torch.library.custom_op("hrnet_hip::mncc_grid_scene", mutates_args=(), device_types="cuda")
def _op_mncc_grid_scene(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                        centres: torch.Tensor, points_per_dim: int, width: float) -> torch.Tensor:
    return mncc_grid_scene(ref, ref_mask, views, view_masks, centres, points_per_dim, width)


@torch.library.custom_op("hrnet_hip::mncc_search_scene", mutates_args=(), device_types="cuda")
def _op_mncc_search_scene(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                          points_per_dim: int, levels: int, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_search_scene(ref, ref_mask, views, view_masks, points_per_dim, levels, radius)


@torch.library.custom_op("hrnet_hip::shift_scene", mutates_args=(), device_types="cuda")
def _op_shift_scene(views: torch.Tensor, view_masks: Optional[torch.Tensor], shifts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_apply_scene(views, view_masks, shifts)


_op_mncc_grid_scene.register_fake(_fake_mncc_grid)
_op_mncc_search_scene.register_fake(_fake_mncc_search)
_op_shift_scene.register_fake(_fake_shift_views)


# The resampler as a differentiable warp (resample_bwd.hip): shift_scene's forward with an autograd formula in the views and the shifts.
# The sampler is linear in the view and C^1 in the shift; `valid` and the masks are piecewise constant and get no gradient.
@torch.library.custom_op("hrnet_hip::warp", mutates_args=(), device_types="cuda")
def _op_warp(views: torch.Tensor, view_masks: Optional[torch.Tensor], shifts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_apply_scene(views, view_masks, shifts)


_op_warp.register_fake(_fake_shift_views)


@torch.library.custom_op("hrnet_hip::warp_backward", mutates_args=(), device_types="cuda")
def _op_warp_backward(views: torch.Tensor, shifts: torch.Tensor, valid: torch.Tensor, d_out: torch.Tensor, need_views: bool,
                      need_shifts: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_views, d_shifts) of mncc_apply_backward; a half that is not needed is not launched and comes back as an empty (0,) tensor."""
    d_views, d_shifts = mncc_apply_backward(views, shifts, valid, d_out, need_views, need_shifts)
    none = views.new_empty((0,), dtype=torch.float32)
    return (d_views if need_views else none), (d_shifts if need_shifts else none.clone())


@_op_warp_backward.register_fake
def _fake_warp_backward(views, shifts, valid, d_out, need_views, need_shifts):
    return (views.new_empty(views.shape if need_views else (0,), dtype=torch.float32),
            views.new_empty(tuple(views.shape[:2]) + (2,) if need_shifts else (0,), dtype=torch.float32))


def _warp_setup(ctx, inputs, output):
    views, _, shifts = inputs
    ctx.save_for_backward(views, shifts, output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _warp_backward(ctx, d_out, _d_valid):
    views, shifts, valid = ctx.saved_tensors
    need_views, need_shifts = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
    if d_out is None or not (need_views or need_shifts):
        return None, None, None
    d_views, d_shifts = torch.ops.hrnet_hip.warp_backward(views, shifts, valid, d_out, need_views, need_shifts)
    return (d_views.to(views.dtype) if need_views else None), None, (d_shifts.to(shifts.dtype) if need_shifts else None)


_op_warp.register_autograd(_warp_backward, setup_context=_warp_setup)


# a shift per block and the resampling by the field (registration_local.hip)
@torch.library.custom_op("hrnet_hip::mncc_search_local", mutates_args=(), device_types="cuda")
def _op_mncc_search_local(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                          init: Optional[torch.Tensor], points_per_dim: int, levels: int, radius: float, block: int,
                          min_valid: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return mncc_search_local(ref, ref_mask, views, view_masks, init, points_per_dim, levels, radius, block, min_valid)


@_op_mncc_search_local.register_fake
def _fake_mncc_search_local(ref, ref_mask, views, view_masks, init, points_per_dim, levels, radius, block, min_valid):
    B, V, H, W = views.shape
    by, bx = mncc_local_blocks(H, W, block)
    return (views.new_empty((B, V, by, bx, 2), dtype=torch.float32), views.new_empty((B, V, by, bx, levels, 3), dtype=torch.float32),
            views.new_empty((B, V, by, bx), dtype=torch.float32))


@torch.library.custom_op("hrnet_hip::shift_field", mutates_args=(), device_types="cuda")
def _op_shift_field(views: torch.Tensor, view_masks: Optional[torch.Tensor], field: torch.Tensor, block: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_apply_field(views, view_masks, field, block)


@_op_shift_field.register_fake
def _fake_shift_field(views, view_masks, field, block):
    return views.new_empty(views.shape, dtype=torch.float32), views.new_empty(views.shape, dtype=torch.float32)


# the masked pyramid and the coarse-to-fine search (registration_pyramid.hip)
@torch.library.custom_op("hrnet_hip::reduce2", mutates_args=(), device_types="cuda")
def _op_reduce2(x: torch.Tensor, mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_reduce2(x, mask)


@_op_reduce2.register_fake
def _fake_reduce2(x, mask):
    shape = (x.shape[0], x.shape[1] // 2, x.shape[2] // 2)
    return x.new_empty(shape, dtype=torch.float32), x.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::mncc_search_scene_from", mutates_args=(), device_types="cuda")
def _op_mncc_search_scene_from(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                               init: Optional[torch.Tensor], points_per_dim: int, levels: int,
                               radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_search_scene_from(ref, ref_mask, views, view_masks, init, points_per_dim, levels, radius)


@_op_mncc_search_scene_from.register_fake
def _fake_mncc_search_scene_from(ref, ref_mask, views, view_masks, init, points_per_dim, levels, radius):
    return _fake_mncc_search(ref, ref_mask, views, view_masks, points_per_dim, levels, radius)


@torch.library.custom_op("hrnet_hip::mncc_search_pyramid", mutates_args=(), device_types="cuda")
def _op_mncc_search_pyramid(ref: torch.Tensor, ref_mask: Optional[torch.Tensor], views: torch.Tensor, view_masks: Optional[torch.Tensor],
                            octaves: int, points_per_dim: int, levels: int, radius: float, coarse_levels: int,
                            refine_radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return mncc_search_pyramid(ref, ref_mask, views, view_masks, octaves, points_per_dim, levels, radius, coarse_levels, refine_radius)


@_op_mncc_search_pyramid.register_fake
def _fake_mncc_search_pyramid(ref, ref_mask, views, view_masks, octaves, points_per_dim, levels, radius, coarse_levels, refine_radius):
    B, V = views.shape[:2]
    return views.new_empty((B, V, 2), dtype=torch.float32), views.new_empty((B, V, octaves + 1, 3), dtype=torch.float32)


@torch.library.custom_op("hrnet_hip::adam_step", mutates_args=("params", "exp_avg", "exp_avg_sq"), device_types="cuda")
def _op_adam_step(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: float, beta1: float,
                  beta2: float, eps: float, weight_decay: float, step: int) -> None:
    """`optimizer.step()` of torch.optim.Adam (train.py:191) on one flat fp32 buffer, in place."""
    adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step)


@torch.library.custom_op("hrnet_hip::grad_sumsq", mutates_args=(), device_types="cuda")
def _op_grad_sumsq(grads: torch.Tensor) -> torch.Tensor:
    """(sum of squares of the finite elements, number of non-finite ones) of a flat fp32 buffer, float64 (2,)"""
    return grad_sumsq(grads)


@_op_grad_sumsq.register_fake
def _fake_grad_sumsq(grads):
    return grads.new_empty((2,), dtype=torch.float64)


@torch.library.custom_op("hrnet_hip::optim_prepare", mutates_args=("ctl",), device_types="cuda")
def _op_optim_prepare(sums: torch.Tensor, ctl: torch.Tensor, group: int, max_norm: float, lr: float, beta1: float, beta2: float) -> None:
    """every group's sums -> the step-control block of one group (norm, clip coefficient, skip, counters, bias corrections), in place"""
    optim_prepare(sums, ctl, group, max_norm, lr, beta1, beta2)


@torch.library.custom_op("hrnet_hip::adam_step_ex", mutates_args=("params", "exp_avg", "exp_avg_sq", "ema"), device_types="cuda")
def _op_adam_step_ex(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, ema: Optional[torch.Tensor],
                     ctl: torch.Tensor, group: int, beta1: float, beta2: float, eps: float, weight_decay: float, decoupled: bool,
                     ema_decay: float) -> None:
    """the clipped, guarded Adam / AdamW step with the EMA of the new weights, on one flat fp32 buffer, in place"""
    adam_step_ex(params, grads, exp_avg, exp_avg_sq, ema, ctl, group, beta1, beta2, eps, weight_decay, decoupled, ema_decay)
