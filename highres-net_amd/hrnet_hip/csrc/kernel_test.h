// Kernel-level hooks for the test suite: the one declaration of every hrn_kt_* entry point.  kernel_test.hip and prof.hip define
// them and include this file, so the compiler holds each definition to its prototype; tests/kt.py binds them, and tests/test_abi.py
// compares that table with these prototypes argument by argument.
//
// The hooks reach the convolution (with its whole epilogue), stem and decoder launchers, the training path's data-gradient and
// weight-gradient launchers, the backward's non-convolution launchers and ShiftNet's passes - BatchNorm statistics / fold / saved
// statistics, the f32 convolution's folded-BatchNorm epilogue, the plane means, the stem / fc adapter passes, fc1 / fc2 and the tail's
// backward - so that each can be checked against fp64 with inputs chosen for it (tests/test_gpu_bf16_train.py,
// tests/test_gpu_shiftnet_bf16.py, tests/test_gpu_kernels_fwd.py, tests/test_gpu_kernels_bwd.py, tests/test_gpu_kernels_shiftnet.py).
// Not part of the public C ABI (include/hrnet_hip.h); same conventions as its entry points: asynchronous on `stream`, 0 or a negative
// error.
#pragma once
#include <stddef.h>

extern "C" {

// bytes of the scratch hrn_kt_conv_wgrad needs on the current device
size_t hrn_kt_wgrad_scratch_bytes(void);

// dw [cout][cin][3][3] f32 += the weight gradient of a cin -> cout conv3x3 (pad 1): x plain [M][H][W][cin] or (x == NULL) the pair
// gather of `stack` [B][pair_vs][H][W][64] (B = M / pair_h); g [M][H][W][cout].  dt HRN_DTYPE_BF16 (x / stack / g one bf16 plane each),
// HRN_DTYPE_BF16X3 (a pair of bf16 planes each, the lo plane directly behind the hi plane, as hrn_conv_dgrad lays them out) or F32.
int hrn_kt_conv_wgrad(int dt, const void* x, const void* stack, int pair_h, int pair_last, int pair_vs, const void* g, int M, int H, int W,
                      int cin, int cout, float* dw, void* scratch, void* stream);

// dx [M][H][W][cin] = the data gradient of a cin -> cout conv3x3 with raw weights w [cout][cin][3][3] f32 at g [M][H][W][cout]
// (+ res [M][H][W][cin] when not NULL), in storage dt; wt / wtp: cin * cout * 9 floats each, zero_bias: 128 zero floats
int hrn_kt_conv_dgrad(int dt, int cin, int cout, const float* w, const void* g, void* dx, const void* res, int M, int H, int W, float* wt,
                      void* wtp, const float* zero_bias, void* stream);

// out [M][H][W][cout] = conv3x3(in) + bias (no activation), in storage dt; in plain [M][H][W][cin] or (in == NULL) the pair gather of
// `stack`; wpk: hrn_launch_conv_pack(dt) of the OIHW weights
int hrn_kt_conv3x3(int dt, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs, const void* wpk,
                   const float* bias, void* out, int M, int H, int W, void* stream);

// One conv3x3 layer with the whole epilogue encoder_impl / fuse_impl (api.hip) set in ConvParams, in storage dt (HRN_DTYPE_BF16,
// BF16X3 or F32): in plain [M][H][W][cin] or (in == NULL) the pair gather of `stack` [B][pair_vs][H][W][64]; the pair descriptor
// (pair_h > 0) also feeds res_mode 2, and pair_last alone res_mode 3's alpha index; wpk: hrn_kt_conv_pack(dt) of the OIHW weights;
// slope: 1 float (device) or NULL; res / res_mode / res_vs, alphas / alpha_vs and the slot output out_h / out_vs as in ConvParams;
// in_lo / stack_lo / out_lo / res_lo: HRN_DTYPE_BF16X3's lo-plane byte offsets.  route 0: hrn_launch_conv3x3 as production calls it
// (r64 / v6 / v6x3); route 1: conv3x3.hip's general kernel, the path HRN_CONV_R64=0 HRN_CONV_V6=0 select.
int hrn_kt_conv3x3_epi(int dt, int route, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs,
                       const void* wpk, const float* bias, const float* slope, const void* res, int res_mode, int res_vs, const float* alphas,
                       int alpha_vs, void* out, int out_h, int out_vs, size_t in_lo, size_t stack_lo, size_t out_lo, size_t res_lo, int M,
                       int H, int W, void* stream);

// The route hrn_kt_conv3x3_epi's launch would take, without launching: hrn_conv3x3_route alone, on the same arguments (no stream; the
// pointers are only compared with NULL) plus the fields that hook does not reach - in_pair as ConvParams has it (hrn_kt_conv3x3_epi
// derives it from in == NULL), scale, relu.  Writes the kernel family ("general" / "r64" / "v6" / "v6x3"), the profiler's family name
// (both static strings) and the persistent grid; a descriptor outside ConvParams' contract is -2 with hrn_last_error() naming the field.
int hrn_kt_conv_route(int dt, int route, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs,
                      const void* wpk, const float* bias, const float* slope, const void* res, int res_mode, int res_vs, const float* alphas,
                      int alpha_vs, void* out, int out_h, int out_vs, size_t in_lo, size_t stack_lo, size_t out_lo, size_t res_lo, int M,
                      int H, int W, int in_pair, const float* scale, int relu, const char** family, const char** prof_name, long* grid);

// out [M][H][W][64] (dt) = the 2 -> 64 stem + PReLU (slope NULL: none) over channel 0 = image m of in0 (img_stride0 floats apart) and
// channel 1 = image m / rep1 of in1, as hrn_launch_stem: sub == NULL reaches stem_mfma_kernel (bf16 / bf16x3), `sub` [M][2] the VALU
// stem_kernel; out_lo: HRN_DTYPE_BF16X3's lo-plane byte offset
int hrn_kt_stem(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1, const float* sub,
                const float* w, const float* bias, const float* slope, void* out, size_t out_lo, int M, int H, int W, void* stream);

// sr [N][S H][S W] f32 = the decoder at scale S of fused [N][H][W][64] (dt; HRN_DTYPE_BF16X3: a pair of bf16 planes, lo fused_lo bytes
// further on), as decoder_impl runs it: w_iokk (64, 64, S, S) f32 packed into wpk first (64 * 64 * S * S floats of scratch), then
// bias / slope / wf / bf f32 (device)
int hrn_kt_decoder(int dt, int scale, const void* fused, size_t fused_lo, const float* w_iokk, void* wpk, const float* bias,
                   const float* slope, const float* wf, const float* bf, float* sr, int N, int H, int W, void* stream);

int hrn_kt_conv_pack(int dt, int cin, int cout, const float* w_oihw, void* packed, void* stream);

// ShiftNet's passes (shiftnet.hip, shiftnet_bwd.hip) in storage dt (HRN_DTYPE_F32 or HRN_DTYPE_BF16) of x / out / dy / dx / g / y.
// BatchNorm statistics of x [npix][C]: scale / shift (C f32 each), running stats updated with `momentum`; partial: 256 x 128 x 2 doubles
int hrn_kt_sn_bn_stats(int dt, const void* x, size_t npix, int C, const float* gamma, const float* beta, float* scale, float* shift,
                       float* running_mean, float* running_var, float momentum, double* partial, void* stream);
// out = [MaxPool2d(2)](ReLU(x * scale + shift)), x [N][H][W][C]
int hrn_kt_sn_bn_act_pool(int dt, const void* x, const float* scale, const float* shift, void* out, int N, int H, int W, int C, int pool,
                          void* stream);
// the BatchNorm + ReLU (+ pool) backward of one layer; stats = {mean, invstd, scale, shift} x 128 f32; partial: 256 x 128 x 2 doubles,
// sums: 128 x 2 doubles
int hrn_kt_sn_bn_bwd(int dt, const void* x, const void* dy, const float* stats, const float* gamma, void* dx, float* dgamma, float* dbeta,
                     int N, int H, int W, int C, int pool, double* partial, double* sums, void* stream);
// din [M][2][H][W] f32 = the stem's input gradient from g [M][H][W][64], w (64, 2, 3, 3) f32
int hrn_kt_sn_stem_dgrad(int dt, const void* g, const float* w, float* din, int M, int H, int W, void* stream);
// xr (B, 32768) f32 <- y [B][256][128] (dropout mask folded in), and back: dy [B][256][128] <- dxr (B, 32768) f32
int hrn_kt_sn_fc_to_ref(int dt, const void* y, const unsigned char* mask, float* xr, int B, void* stream);
int hrn_kt_sn_fc_from_ref(int dt, const float* dxr, const unsigned char* mask, void* dy, int B, void* stream);

// ---- ShiftNet's remaining passes (tests/test_gpu_kernels_shiftnet.py), each the production launcher as api.hip / shiftnet_bwd.hip call it
// mean / invstd (C f32 each) from the `partial` sums hrn_kt_sn_bn_stats left
int hrn_kt_sn_bn_save_stats(const double* partial, size_t npix, int C, float* mean, float* invstd, void* stream);
// eval mode's folded BatchNorm: scale / shift from the running statistics (conv_bias NULL: none)
int hrn_kt_sn_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, const float* conv_bias, float* scale,
                      float* shift, int C, void* stream);
// out [M][H][W][cout] f32 = ReLU(conv3x3(in) * scale + shift): the f32 convolution with eval mode's folded-BatchNorm epilogue
int hrn_kt_sn_conv_bn_relu(int cin, int cout, const float* in, const void* wpk, const float* scale, const float* shift, float* out, int M, int H,
                           int W, void* stream);
// mean [planes] of x [planes][hw], and out = g - means[plane]
int hrn_kt_sn_plane_mean(const float* x, float* mean, int planes, size_t hw, void* stream);
int hrn_kt_sn_sub_plane_mean(const float* g, const float* means, float* out, int planes, size_t hw, void* stream);
// y (B, 1024) = ReLU(bias + xr w^T), xr (B, 32768), w (1024, 32768); partial: hrn_kt_sn_fc1_partial_bytes() of scratch
size_t hrn_kt_sn_fc1_partial_bytes(void);
int hrn_kt_sn_fc1(const float* xr, const float* w, const float* bias, float* y, int B, float* partial, void* stream);
// theta (B, 2) = y w2^T, w2 (2, 1024)
int hrn_kt_sn_fc2(const float* y, const float* w2, float* theta, int B, void* stream);
// the tail's backward (dw2 / db1 NULL: frozen)
int hrn_kt_sn_fc2_bwd(const float* dtheta, const float* y1, const float* w2, float* dz1, float* dw2, float* db1, int B, void* stream);
int hrn_kt_sn_fc1_bwd_w(const float* dz1, const float* xr, float* dw1, int B, void* stream);
int hrn_kt_sn_fc1_bwd_x(const float* dz1, const float* w1, float* dxr, int B, void* stream);

// ---- the backward's non-convolution launchers (tests/test_gpu_kernels_bwd.py), each called as train.hip / api.hip call it.  Activation
// and gradient tensors in storage dt; HRN_DTYPE_BF16X3: the lo plane directly behind the hi plane (each kernel derives its offset from
// the element count).  scratch: hrn_kt_wgrad_scratch_bytes() bytes unless said otherwise.
// g [rows][C] = dy * PReLU'(x), dslope[0] += sum dy min(x, 0), db[c] += sum_rows g (db / dslope NULL: a frozen parameter)
int hrn_kt_prelu_bwd_bias(int dt, const void* dy, const void* y, const void* xpre, const float* slope, void* g, size_t rows, int C,
                          float* dslope, float* db, void* scratch, void* stream);
// db[c] += sum_rows g[row][c]
int hrn_kt_colsum(int dt, const void* g, size_t rows, int C, float* db, void* scratch, void* stream);
// o = a + b, n elements
int hrn_kt_add(int dt, const void* a, const void* b, void* o, size_t n, void* stream);
// the fusion level's helpers: stack [B][n_in][hw][64], f / dsn / out / df [B * half][hw][64], dz [B * half][hw][128], ds [B][n_in][hw][64]
int hrn_kt_fuse_update(int dt, const void* stack, int n_in, const void* f, const float* alphas, int alpha_vs, int pair_last, int half,
                       int alpha_residual, void* out, size_t hw, int B, void* stream);
// t2 [B * half][hw][128] = cat(view v, view pair_last - v of stack) + u: the training forward's z + u of a fusion level
int hrn_kt_pair_add(int dt, const void* stack, int n_in, int half, int pair_last, const void* u, void* t2, size_t hw, int B, void* stream);
int hrn_kt_fuse_df(int dt, const void* dsn, const float* alphas, int alpha_vs, int pair_last, int half, int alpha_residual, void* df, size_t hw,
                   int B, void* stream);
int hrn_kt_fuse_scatter(int dt, const void* dsn, const void* dz, int n_in, int half, int pair_last, int alpha_residual, void* ds, size_t hw,
                        int B, void* stream);
// d_alphas[b][pair_last - v] = sum dsn * f of image b * half + v; scratch: hrn_kt_alpha_grad_scratch_bytes(B * half) bytes
size_t hrn_kt_alpha_grad_scratch_bytes(int nimg);
int hrn_kt_alpha_grad(int dt, const void* dsn, const void* f, int half, int pair_last, float* d_alphas, int B, int V, size_t hw, void* scratch,
                      size_t scratch_bytes, void* stream);
// dw [64][2][3][3] += the stem's weight gradient; sub NULL: hrn_launch_stem_wgrad (HRNet), else hrn_launch_stem_wgrad_sub (ShiftNet)
int hrn_kt_stem_wgrad(int dt, const float* in0, size_t stride0, const float* in1, int rep1, size_t stride1, const float* sub, const void* g,
                      int M, int H, int W, float* dw, void* scratch, void* stream);
// d_lrs [B][V][H][W] = the stem's input gradient with the median routing; wt: 64 * 18 floats of scratch
int hrn_kt_stem_dgrad_route(int dt, const void* dA, const float* w, float* wt, const float* lrs, const float* ref, float* d_lrs, int B, int V,
                            int H, int W, void* stream);
// the same data gradient with the reference frame given from outside (hrn_launch_stem_dgrad_ref, no routing): d_lrs [B][V][H][W] = channel 0
// per view, d_ref [B][H][W] = channel 1 summed over the sample's V views in view order; either may be NULL (not wanted, not written), both
// NULL is -2 before any launch; dA [B V][H][W][64] in storage dt is only read; wt: 64 * 18 floats of scratch; tiles B < 2^31 or -2
int hrn_kt_stem_dgrad_ref(int dt, const void* dA, const float* w, float* wt, float* d_lrs, float* d_ref, int B, int V, int H, int W,
                          void* stream);
// out [M][H][W][64] (dt) = the stem's pre-activation, only if only_if_nonpos[0] <= 0
int hrn_kt_stem_pre(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1, const float* w,
                    const float* bias, void* out, int M, int H, int W, const float* only_if_nonpos, void* stream);
// the f32 decoder backward at scale S: writes d_fused, accumulates the five gradients (NULL: a frozen parameter)
int hrn_kt_decoder_bwd(int scale, const float* fused, const float* d_sr, const float* wd, const float* bd, const float* ad, const float* wf,
                       float* d_fused, float* dwd, float* dbd, float* dad, float* dwf, float* dbf, int N, int H, int W, void* scratch,
                       void* stream);
int hrn_kt_planes_to_f32(const void* hi, size_t lo_off, float* out, size_t n, void* stream);
int hrn_kt_f32_to_planes(const float* in, void* hi, size_t lo_off, size_t n, void* stream);
// ref [B][H][W] = the lower median of lrs[b, :min(V, 9)]
int hrn_kt_median(const float* lrs, float* ref, int B, int V, int H, int W, void* stream);

// ---- the host-side launch counters of prof.h (prof.hip): launches of counter `name` since the last reset, -1 for a name it does not know
long hrn_kt_launch_count(const char* name);
void hrn_kt_launch_count_reset(void);

}  // extern "C"
