// Launchers of the backward building blocks (backward.hip).  dt, always the first argument, = HRN_F32, HRN_BF16 or HRN_BF16X3 is the
// storage of every `void*` tensor: f32, one bf16 plane (the bf16 training mode), or a pair of bf16 planes (bf16x3; hi, then lo directly
// behind it: a tensor of n elements has its lo plane 2 n bytes further on).  A `float*` is f32 whatever dt says: parameters, their
// gradients, the network's inputs and outputs.  No argument has a default.  Same conventions as kernels.h: asynchronous on `stream`, no
// allocation, no synchronisation; gradients are ACCUMULATED (+=) into their destination, like autograd's .grad.
#pragma once
#include "common.h"

// bytes of the `scratch` buffer the launchers below share (wgrad partial slabs, reduction partials)
size_t hrn_bwd_scratch_bytes(int num_cus);

// PReLU backward and the bias gradient of the convolution in front of it, in one pass: g = dy * PReLU'(x) ([rows][C], C in
// {64, 128}; may alias dy), dslope[0] += sum dy * min(x, 0), db[c] += sum_rows g[row][c].  x comes from the stored post-activation
// y when slope[0] > 0 and from the pre-activation xpre otherwise (decided on the device; the caller recomputes xpre with a launch
// gated the same way: ConvParams::only_if_nonpos)
int hrn_launch_prelu_bwd_bias(int dt, const void* dy, const void* y, const void* xpre, const float* slope, void* g, size_t rows, int C,
                              float* dslope, float* db, void* scratch, hipStream_t s);
// db[c] += sum_rows g[row][c], C in {64, 128}
int hrn_launch_colsum(int dt, const void* g, size_t rows, int C, float* db, void* scratch, hipStream_t s);
// wt[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]: the OIHW tensor whose forward convolution is the data gradient
int hrn_launch_dgrad_weights(const float* w, float* wt, int cin, int cout, hipStream_t s);
// dw[co][ci][3][3] += sum g (x) shifted x; x plain [M][H][W][cin] or (in_pair) the pair gather of `stack` [M / pair_h][pair_vs][H][W][64]
// (cin = 128); x / stack and g [M][H][W][cout] in storage dt.  Picks one of the three launchers below (bf16x3: with the lo planes
// directly behind the hi planes)
int hrn_launch_conv_wgrad(int dt, const void* x, const void* stack, int in_pair, int pair_h, int pair_last, int pair_vs, const void* g,
                          int M, int H, int W, int cin, int cout, float* dw, void* scratch, int num_cus, hipStream_t s);
// fp32 (backward.hip)
int hrn_launch_conv_wgrad_f32(const float* x, const float* stack, int in_pair, int pair_h, int pair_last, int pair_vs, const float* g,
                              int M, int H, int W, int cin, int cout, float* dw, void* scratch, int num_cus, hipStream_t s);
// the bf16x3 training mode (wgrad_x3.hip): x / stack and g are pairs of bf16 planes, x_lo / g_lo the byte offsets of their lo planes
int hrn_launch_conv_wgrad_x3(const void* x, const void* stack, size_t x_lo, int in_pair, int pair_h, int pair_last, int pair_vs, const void* g,
                             size_t g_lo, int M, int H, int W, int cin, int cout, float* dw, void* scratch, int num_cus, hipStream_t s);
// the same in the bf16 training mode (wgrad_x3.hip): x / stack and g are one bf16 plane each, one MFMA per product, fp32 accumulation
int hrn_launch_conv_wgrad_bf16(const void* x, const void* stack, int in_pair, int pair_h, int pair_last, int pair_vs, const void* g, int M,
                               int H, int W, int cin, int cout, float* dw, void* scratch, int num_cus, hipStream_t s);
// dW[co][ci][tap] += sum over workgroups of the partial slabs [nblk][9][64][64] of one (cout chunk, cin chunk) pair, fixed order
int hrn_launch_wgrad_finish(const float* partial, int nblk, float* dw, int cin, int co_chunk, int ci_chunk, hipStream_t s);
// stem 2 -> 64: in0 = image m (stride0 floats apart), in1 = plane m / rep1; dw [64][2][3][3]
int hrn_launch_stem_wgrad(int dt, const float* in0, size_t stride0, const float* in1, int rep1, size_t stride1, const void* g, int M, int H,
                          int W, float* dw, void* scratch, int num_cus, hipStream_t s);
// the same with `sub` [M][2] subtracted from the in-image pixels of the two planes first (ShiftNet's mean-free input)
int hrn_launch_stem_wgrad_sub(int dt, const float* in0, size_t stride0, const float* in1, int rep1, size_t stride1, const float* sub,
                              const void* g, int M, int H, int W, float* dw, void* scratch, int num_cus, hipStream_t s);
int hrn_launch_add(int dt, const void* a, const void* b, void* o, size_t n, hipStream_t s);
// fusion level helpers (HRNet.py:113-132): forward update of the kept views, and the two backward maps
int hrn_launch_fuse_update(int dt, const void* stack, int n_in, const void* f, const float* alphas, int alpha_vs, int pair_last, int half,
                           int alpha_residual, void* out, size_t hw, int B, hipStream_t s);
// t2 = z + u for the pair gather z = cat(view i, view pair_last - i) of stack [B][n_in][hw][64]; u, t2 [B * half][hw][128] (train.hip)
int hrn_launch_pair_add(int dt, const void* stack, int n_in, int half, int pair_last, const void* u, void* t2, size_t hw, int B, hipStream_t s);
int hrn_launch_fuse_df(int dt, const void* dsn, const float* alphas, int alpha_vs, int pair_last, int half, int alpha_residual, void* df,
                       size_t hw, int B, hipStream_t s);
int hrn_launch_fuse_scatter(int dt, const void* dsn, const void* dz, int n_in, int half, int pair_last, int alpha_residual, void* ds,
                            size_t hw, int B, hipStream_t s);
// Decoder backward (HRNet.py:147-156,167-169), S = scale in {2, 3, 4}: fused [N][H][W][64] f32, d_sr [N][S H][S W]; reference-layout
// parameters wd (64,64,S,S) = (Cin,Cout,kH,kW), bd (64), ad (1), wf (64), bf (1).  Writes d_fused; accumulates the five gradients.
int hrn_launch_decoder_bwd(const float* fused, const float* d_sr, const float* wd, const float* bd, const float* ad, const float* wf,
                           float* d_fused, float* dwd, float* dbd, float* dad, float* dwf, float* dbf, int N, int H, int W,
                           void* scratch, int num_cus, hipStream_t s, int scale);
// bytes of the launcher's `scratch` (0 for an unsupported scale); no larger than hrn_bwd_scratch_bytes for any scale
size_t hrn_decoder_bwd_scratch_bytes(int num_cus, int scale);
// dx = conv3x3(g, W^T with taps flipped) (+ res): the data gradient of a cin -> cout convolution with raw weights
// w [cout][cin][3][3], on the forward kernel of dt (g, dx, res in that storage).  wt / wtp: scratch for the transposed OIHW tensor and
// its packed form (cin*cout*9 floats each); zero_bias: max(cin, cout) zero floats.
int hrn_conv_dgrad(int dt, int cin, int cout, const float* w, const void* g, void* dx, const void* res, int M, int H, int W, float* wt,
                   void* wtp, const float* zero_bias, hipStream_t s);
// Input gradients (input_grad.hip), WRITTEN rather than accumulated.  Stem data gradient plus the median routing: dA [B*V][H][W][64]
// (dt) is the stem's pre-activation gradient, w the raw stem weights (64, 2, 3, 3), ref [B][H][W] the forward's lower median of
// lrs[b, :min(V, 9)]; d_lrs [B][V][H][W] gets channel 0 of the input gradient per view plus, at one view per pixel (the lowest-indexed
// of the first min(V, 9) views equal to the median), channel 1 summed over the sample's views.
// wt: scratch for 64 * 18 floats (the weights transposed tap-major)
int hrn_launch_stem_dgrad_route(int dt, const void* dA, const float* w, float* wt, const float* lrs, const float* ref, float* d_lrs, int B,
                                int V, int H, int W, hipStream_t s);
// The same data gradient for a reference frame that came from outside (no median to route to): d_lrs [B][V][H][W] gets channel 0 alone,
// d_ref [B][H][W] channel 1 summed over the sample's views in view order.  Either may be null (not both)
int hrn_launch_stem_dgrad_ref(int dt, const void* dA, const float* w, float* wt, float* d_lrs, float* d_ref, int B, int V, int H, int W,
                              hipStream_t s);
// One fusion level's alpha gradient: d_alphas[b][pair_last - v] = sum over pixels and channels of dsn * f, image b * half + v of the
// level's outputs ([B*half][hw][64] each, dt); uses hrn_alpha_grad_scratch_bytes(B * half) bytes of `scratch`
size_t hrn_alpha_grad_scratch_bytes(int nimg);
int hrn_launch_alpha_grad(int dt, const void* dsn, const void* f, int half, int pair_last, float* d_alphas, int B, int V, size_t hw,
                          void* scratch, size_t scratch_bytes, hipStream_t s);
