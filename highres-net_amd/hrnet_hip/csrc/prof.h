// Built-in kernel timing: when enabled (hrn_profile_enable), every launcher brackets its kernel with a hipEvent pair
// on the launch stream and files it under a kernel-family name together with the launch's algorithmic FLOPs and
// bytes.  bench.py reads the totals back (hrn_profile_get) to state achieved TFLOP/s / GB/s per family against the
// gfx950 roofline.  Disabled (the default) it costs one predictable branch per launch.
#pragma once
#include <hip/hip_runtime.h>

struct HrnProfScope {
    int rec;
    hipStream_t stream;
    HrnProfScope(const char* family, double flops, double bytes, hipStream_t s);
    ~HrnProfScope();
};

// Host-side launch counters for the backward's kernels that carry no HrnProfScope (the profiler's families are part of bench.py's
// output, so these stay out of it).  One relaxed atomic increment per launch, always on; read and reset only through the test
// hooks hrn_kt_launch_count / hrn_kt_launch_count_reset (kernel_test.hip).
enum HrnLaunchCounter {
    HRN_LC_CONV_WGRAD_F32,      // conv_wgrad_kernel (backward.hip; one per 64 x 64 chunk pair)
    HRN_LC_STEM_WGRAD,          // stem_wgrad_kernel
    HRN_LC_PRELU_BWD,           // prelu_bwd_bias_kernel
    HRN_LC_BIAS_FINISH,         // colsum_finish_kernel (a bias gradient)
    HRN_LC_SLOPE_FINISH,        // scalar_finish_kernel (a PReLU slope gradient)
    HRN_LC_CONV_DGRAD,          // hrn_conv_dgrad (the forward conv on transposed weights, every dtype)
    HRN_LC_DECODER_BWD,         // decoder_bwd_kernel
    HRN_LC_DECODER_BWD_FINISH,  // decoder_bwd_finish_kernel
    HRN_LC_FUSE_SCATTER,        // fuse_scatter_kernel
    HRN_LC_SN_BN_BWD,           // ShiftNet's BatchNorm backward (reduce + finish + apply)
    HRN_LC_FC2_BWD,             // fc2_bwd_kernel
    HRN_LC_FC1_BWD_W,           // fc1_bwd_w_kernel
    HRN_LC_FC1_BWD_X,           // fc1_bwd_x_kernel
    HRN_LC_CONV_GENERAL,        // conv3x3_kernel (conv3x3.hip's general kernel: every f32 layer, and the bf16 layers r64 / v6 decline -
                                // their plain layers share its profiler family names, so only this tells the routes apart)
    HRN_LC_COUNT
};
void hrn_count_launch(int which);
