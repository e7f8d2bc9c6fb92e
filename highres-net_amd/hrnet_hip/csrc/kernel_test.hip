// Kernel-level hooks for the test suite (tests/test_gpu_bf16_train.py, tests/test_gpu_shiftnet_bf16.py): the training path's convolution,
// data-gradient and weight-gradient launchers and ShiftNet's BatchNorm / stem / fc adapter passes called on their own, so that each can be checked against fp64 with inputs chosen for it.  Not part of the
// public C ABI (include/hrnet_hip.h); same conventions as its entry points: asynchronous on `stream`, 0 or a negative error.
#include <string.h>
#include "kernels.h"
#include "backward.h"

extern "C" {

// bytes of the scratch hrn_kt_conv_wgrad needs on the current device
size_t hrn_kt_wgrad_scratch_bytes(void) { return hrn_bwd_scratch_bytes(hrn_device_cus()); }

// dw [cout][cin][3][3] f32 += the weight gradient of a cin -> cout conv3x3 (pad 1): x plain [M][H][W][cin] or (x == NULL) the pair
// gather of `stack` [B][pair_vs][H][W][64]; g [M][H][W][cout].  dt HRN_DTYPE_BF16 (x / stack / g one bf16 plane each) or F32.
int hrn_kt_conv_wgrad(int dt, const void* x, const void* stack, int pair_h, int pair_last, int pair_vs, const void* g, int M, int H, int W,
                      int cin, int cout, float* dw, void* scratch, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int cus = hrn_device_cus();
    if (dt == HRN_BF16) return hrn_launch_conv_wgrad_bf16(x, stack, x ? 0 : 1, pair_h, pair_last, pair_vs, g, M, H, W, cin, cout, dw, scratch, cus, s);
    HRN_CHECK(dt == HRN_F32, -2, "hrn_kt_conv_wgrad: dtype %d", dt);
    return hrn_launch_conv_wgrad((const float*)x, (const float*)stack, x ? 0 : 1, pair_h, pair_last, pair_vs, (const float*)g, M, H, W, cin, cout,
                                 dw, scratch, cus, s);
}

// dx [M][H][W][cin] = the data gradient of a cin -> cout conv3x3 with raw weights w [cout][cin][3][3] f32 at g [M][H][W][cout]
// (+ res [M][H][W][cin] when not NULL), in storage dt; wt / wtp: cin * cout * 9 floats each, zero_bias: 128 zero floats
int hrn_kt_conv_dgrad(int dt, int cin, int cout, const float* w, const void* g, void* dx, const void* res, int M, int H, int W, float* wt,
                      void* wtp, const float* zero_bias, void* stream) {
    return hrn_conv_dgrad(cin, cout, w, (const float*)g, (float*)dx, (const float*)res, M, H, W, wt, wtp, zero_bias, (hipStream_t)stream, dt);
}

// out [M][H][W][cout] = conv3x3(in) + bias (no activation), in storage dt; in plain [M][H][W][cin] or (in == NULL) the pair gather of
// `stack`; wpk: hrn_launch_conv_pack(dt) of the OIHW weights
int hrn_kt_conv3x3(int dt, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs, const void* wpk,
                   const float* bias, void* out, int M, int H, int W, void* stream) {
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.M = M; p.H = H; p.W = W;
    p.in = in; p.out = out; p.wpk = wpk; p.bias = bias;
    if (!in) { p.in_pair = 1; p.stack = stack; p.pair_h = pair_h; p.pair_last = pair_last; p.pair_vs = pair_vs; }
    return hrn_launch_conv3x3(dt, cin, cout, p, (hipStream_t)stream);
}

int hrn_kt_conv_pack(int dt, int cin, int cout, const float* w_oihw, void* packed, void* stream) {
    return hrn_launch_conv_pack(dt, cin, cout, w_oihw, packed, (hipStream_t)stream);
}

// ShiftNet's passes (shiftnet.hip, shiftnet_bwd.hip) in storage dt (HRN_DTYPE_F32 or HRN_DTYPE_BF16) of x / out / dy / dx / g / y.
// BatchNorm statistics of x [npix][C]: scale / shift (C f32 each), running stats updated with `momentum`; partial: 256 x 128 x 2 doubles
int hrn_kt_sn_bn_stats(int dt, const void* x, size_t npix, int C, const float* gamma, const float* beta, float* scale, float* shift,
                       float* running_mean, float* running_var, float momentum, double* partial, void* stream) {
    return hrn_launch_bn_stats((const float*)x, npix, C, gamma, beta, 1e-5f, scale, shift, running_mean, running_var, momentum, partial, 256,
                               (hipStream_t)stream, dt);
}
// out = [MaxPool2d(2)](ReLU(x * scale + shift)), x [N][H][W][C]
int hrn_kt_sn_bn_act_pool(int dt, const void* x, const float* scale, const float* shift, void* out, int N, int H, int W, int C, int pool,
                          void* stream) {
    return hrn_launch_bn_act_pool((const float*)x, scale, shift, (float*)out, N, H, W, C, pool, (hipStream_t)stream, dt);
}
// the BatchNorm + ReLU (+ pool) backward of one layer; stats = {mean, invstd, scale, shift} x 128 f32; partial: 256 x 128 x 2 doubles,
// sums: 128 x 2 doubles
int hrn_kt_sn_bn_bwd(int dt, const void* x, const void* dy, const float* stats, const float* gamma, void* dx, float* dgamma, float* dbeta,
                     int N, int H, int W, int C, int pool, double* partial, double* sums, void* stream) {
    return hrn_launch_sn_bn_bwd((const float*)x, (const float*)dy, stats, gamma, (float*)dx, dgamma, dbeta, N, H, W, C, pool, partial, sums,
                                (hipStream_t)stream, dt);
}
// din [M][2][H][W] f32 = the stem's input gradient from g [M][H][W][64], w (64, 2, 3, 3) f32
int hrn_kt_sn_stem_dgrad(int dt, const void* g, const float* w, float* din, int M, int H, int W, void* stream) {
    return hrn_launch_sn_stem_dgrad((const float*)g, w, din, M, H, W, (hipStream_t)stream, dt);
}
// xr (B, 32768) f32 <- y [B][256][128] (dropout mask folded in), and back: dy [B][256][128] <- dxr (B, 32768) f32
int hrn_kt_sn_fc_to_ref(int dt, const void* y, const unsigned char* mask, float* xr, int B, void* stream) {
    return hrn_launch_fc_to_ref((const float*)y, mask, xr, B, (hipStream_t)stream, dt);
}
int hrn_kt_sn_fc_from_ref(int dt, const float* dxr, const unsigned char* mask, void* dy, int B, void* stream) {
    return hrn_launch_fc_from_ref(dxr, mask, (float*)dy, B, (hipStream_t)stream, dt);
}

}  // extern "C"
