"""The test suite's binding of the kernel-level hooks hrn_kt_* (highres-net_amd/hrnet_hip/csrc/kernel_test.h): one ctypes table for all of
them, typed at once by lib(), plus what every caller of a hook needs - pointers, the stream, the dtype constants - and the launch
counters.  tests/test_abi.py compares SIGNATURES with the header argument by argument; argtypes / restype are assigned nowhere else
under tests/."""
import ctypes
import functools

import torch

from hrnet_hip import binding

F32, BF16, BF16X3 = 0, 1, 2

# name -> (restype, argtypes), in the order of kernel_test.h
i, vp, sz, fl = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
SIGNATURES = {
    "hrn_kt_wgrad_scratch_bytes": (sz, []),
    "hrn_kt_conv_wgrad": (i, [i, vp, vp, i, i, i, vp, i, i, i, i, i, vp, vp, vp]),
    "hrn_kt_conv_dgrad": (i, [i, i, i, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp]),
    "hrn_kt_conv3x3": (i, [i, i, i, vp, vp, i, i, i, vp, vp, vp, i, i, i, vp]),
    "hrn_kt_conv3x3_epi": (i, [i, i, i, i, vp, vp, i, i, i, vp, vp, vp, vp, i, i, vp, i, vp, i, i, sz, sz, sz, sz, i, i, i, vp]),
    "hrn_kt_conv_route": (i, [i, i, i, i, vp, vp, i, i, i, vp, vp, vp, vp, i, i, vp, i, vp, i, i, sz, sz, sz, sz, i, i, i, i, vp, i, vp, vp, vp]),
    "hrn_kt_stem": (i, [i, vp, sz, vp, i, sz, vp, vp, vp, vp, vp, sz, i, i, i, vp]),
    "hrn_kt_decoder": (i, [i, i, vp, sz, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]),
    "hrn_kt_conv_pack": (i, [i, i, i, vp, vp, vp]),
    # ShiftNet's passes
    "hrn_kt_sn_bn_stats": (i, [i, vp, sz, i, vp, vp, vp, vp, vp, vp, fl, vp, vp]),
    "hrn_kt_sn_bn_act_pool": (i, [i, vp, vp, vp, vp, i, i, i, i, i, vp]),
    "hrn_kt_sn_bn_bwd": (i, [i, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp]),
    "hrn_kt_sn_stem_dgrad": (i, [i, vp, vp, vp, i, i, i, vp]),
    "hrn_kt_sn_fc_to_ref": (i, [i, vp, vp, vp, i, vp]),
    "hrn_kt_sn_fc_from_ref": (i, [i, vp, vp, vp, i, vp]),
    "hrn_kt_sn_bn_save_stats": (i, [vp, sz, i, vp, vp, vp]),
    "hrn_kt_sn_bn_fold": (i, [vp, vp, vp, vp, vp, vp, vp, i, vp]),
    "hrn_kt_sn_conv_bn_relu": (i, [i, i, vp, vp, vp, vp, vp, i, i, i, vp]),
    "hrn_kt_sn_plane_mean": (i, [vp, vp, i, sz, vp]),
    "hrn_kt_sn_sub_plane_mean": (i, [vp, vp, vp, i, sz, vp]),
    "hrn_kt_sn_fc1_partial_bytes": (sz, []),
    "hrn_kt_sn_fc1": (i, [vp, vp, vp, vp, i, vp, vp]),
    "hrn_kt_sn_fc2": (i, [vp, vp, vp, i, vp]),
    "hrn_kt_sn_fc2_bwd": (i, [vp, vp, vp, vp, vp, vp, i, vp]),
    "hrn_kt_sn_fc1_bwd_w": (i, [vp, vp, vp, i, vp]),
    "hrn_kt_sn_fc1_bwd_x": (i, [vp, vp, vp, i, vp]),
    # the backward's non-convolution launchers
    "hrn_kt_prelu_bwd_bias": (i, [i, vp, vp, vp, vp, vp, sz, i, vp, vp, vp, vp]),
    "hrn_kt_colsum": (i, [i, vp, sz, i, vp, vp, vp]),
    "hrn_kt_add": (i, [i, vp, vp, vp, sz, vp]),
    "hrn_kt_fuse_update": (i, [i, vp, i, vp, vp, i, i, i, i, vp, sz, i, vp]),
    "hrn_kt_pair_add": (i, [i, vp, i, i, i, vp, vp, sz, i, vp]),
    "hrn_kt_fuse_df": (i, [i, vp, vp, i, i, i, i, vp, sz, i, vp]),
    "hrn_kt_fuse_scatter": (i, [i, vp, vp, i, i, i, i, vp, sz, i, vp]),
    "hrn_kt_alpha_grad_scratch_bytes": (sz, [i]),
    "hrn_kt_alpha_grad": (i, [i, vp, vp, i, i, vp, i, i, sz, vp, sz, vp]),
    "hrn_kt_stem_wgrad": (i, [i, vp, sz, vp, i, sz, vp, vp, i, i, i, vp, vp, vp]),
    "hrn_kt_stem_dgrad_route": (i, [i, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]),
    "hrn_kt_stem_dgrad_ref": (i, [i, vp, vp, vp, vp, vp, i, i, i, i, vp]),
    "hrn_kt_stem_pre": (i, [i, vp, sz, vp, i, sz, vp, vp, vp, i, i, i, vp, vp]),
    "hrn_kt_decoder_bwd": (i, [i] + [vp] * 12 + [i, i, i, vp, vp]),
    "hrn_kt_planes_to_f32": (i, [vp, sz, vp, sz, vp]),
    "hrn_kt_f32_to_planes": (i, [vp, vp, sz, sz, vp]),
    "hrn_kt_median": (i, [vp, vp, i, i, i, i, vp]),
    # the launch counters
    "hrn_kt_launch_count": (ctypes.c_long, [ctypes.c_char_p]),
    "hrn_kt_launch_count_reset": (None, []),
}
del i, vp, sz, fl


@functools.lru_cache(maxsize=None)
def lib():
    """the library as binding.load_library() types it, with every hook typed too"""
    lib = binding.load_library()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


COUNTERS = ("conv_wgrad_f32", "stem_wgrad", "prelu_bwd", "bias_finish", "slope_finish", "conv_dgrad", "decoder_bwd", "decoder_bwd_finish",
            "fuse_scatter", "sn_bn_bwd", "fc2_bwd", "fc1_bwd_w", "fc1_bwd_x", "conv_general")


def _launches(fn):
    """Run fn() with the launch counters reset and the profiler on -> {name: launches} of both (profiled families as 'prof:<family>')."""
    torch.cuda.synchronize()
    lib().hrn_kt_launch_count_reset()
    binding.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        binding.profile_enable(False)
    got = {c: lib().hrn_kt_launch_count(c.encode()) for c in COUNTERS}
    assert all(v >= 0 for v in got.values()), got
    for name, row in binding.profile_read().items():
        got["prof:" + name] = row["launches"]
    return got, out
