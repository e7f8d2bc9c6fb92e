// Internal launcher declarations (one per kernel family).  All launch asynchronously on `stream`, allocate
// nothing and never synchronise (graph-capturable); they return 0 or a negative error with hrn_set_error() set.
// A launcher whose tensors' storage varies takes dt (HRN_F32 / HRN_BF16 / HRN_BF16X3) first and those tensors as `void*`; a `float*` is
// always f32.  No argument has a default.
#pragma once
#include "common.h"
#include "conv3x3.h"

// ---- composite.hip: the masked lower median of the first min(V, n_ref) views and the filled views (masks / alphas / count / filled may be null)
int hrn_launch_masked_composite(const float* views, const float* masks, const float* alphas, int B, int V, int H, int W, int n_ref, float* ref,
                                float* count, float* filled, hipStream_t stream);
// ---- stem.hip
int hrn_launch_median(const float* lrs, float* ref, int B, int V, int H, int W, hipStream_t stream);
int hrn_launch_stem(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1,
                    const float* sub, const float* w, const float* bias, const float* slope, void* out,
                    int M, int H, int W, hipStream_t stream, size_t out_lo);       // out_lo: HRN_BF16X3's lo-plane byte offset (else 0)
int hrn_launch_planes_to_f32(const void* hi, size_t lo_off, float* out, size_t n, hipStream_t stream);
int hrn_launch_f32_to_planes(const float* in, void* hi, size_t lo_off, size_t n, hipStream_t stream);
int hrn_launch_stem_pre(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1, const float* w,
                        const float* bias, void* out, int M, int H, int W, const float* only_if_nonpos, hipStream_t stream);
int hrn_launch_plane_mean(const float* x, float* mean, int planes, size_t hw, hipStream_t stream);

// ---- decoder.hip
// fused [N][HW][64] (dt) -> sr [N][S H][S W] f32, S = scale in {2, 3, 4}.  wpk: packed deconv weights (hrn_launch_decoder_pack of
// the same scale), bias/slope/wf/bf f32.  fused_lo: HRN_BF16X3's lo-plane byte offset (else 0)
int hrn_launch_decoder(int dt, const void* fused, const void* wpk, const float* bias, const float* slope,
                       const float* wf, const float* bf, float* sr, int N, int H, int W, hipStream_t stream, size_t fused_lo, int scale);
// w_iokk (64, 64, S, S)
int hrn_launch_decoder_pack(int dt, const float* w_iokk, void* packed, hipStream_t stream, int scale);

// ---- lanczos.hip
int hrn_launch_lanczos_taps(const float* d, int n, float* taps, hipStream_t stream);
int hrn_launch_lanczos_shift(const float* img, const float* shift, int b, int c, int H, int W, float* out, hipStream_t stream);
// ---- lanczos_bwd.hip: d_img (may be null) = adjoint of the shift, d_shift [c][2] (may be null) += gradient through the taps
size_t hrn_lanczos_bwd_workspace_bytes_impl(int b, int c, int H, int W);
int hrn_launch_lanczos_shift_bwd(const float* img, const float* shift, const float* dout, int b, int c, int H, int W, float* d_img,
                                 float* d_shift, void* ws, hipStream_t stream);

// ---- losses.hip
int hrn_launch_masked_cmse(const float* srs, const float* hrs, const float* maps, int B, int S, int crop, int metric, float* out,
                           hipStream_t stream);
// differentiable registered-loss tail (train.py:78-87, :183-187): forward keeps stats[B][4] = {n, bias, cMSE, 0} for the backward
size_t hrn_loss_train_workspace_bytes_impl(int B);
int hrn_launch_loss_train(const float* srs, const float* hrs, const float* maps, int B, int S, int crop, int metric, float* out,
                          double* stats, double* partial, hipStream_t stream);
int hrn_launch_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                             int S, int crop, int metric, float* d_srs, hipStream_t stream);
int hrn_launch_shift_cpsnr(const float* srs, const float* hrs, const float* maps, int B, int S, int border, int clip,
                           double* scores, float* out, hipStream_t stream);

// ---- shift_loss.hip: the shift-searched cMSE / cPSNR as a training tail (Evaluator.py:52-73 over train.py:66-87), rectangular frames,
// border 0..8.  Forward: per-tile fp64 sums at every offset into `partial`, fixed-order finish -> out [B], stats [B][4] = {n*, bias*,
// cMSE*, k*} of the selected offset k* = u (2 border + 1) + v (n* = 0, k* = -1, out NaN without a clear pixel).  Backward: d_srs [B][H][W],
// every element written, through the selected offset only.
size_t hrn_shift_loss_workspace_bytes_impl(int B, int H, int W, int border);
int hrn_launch_shift_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int metric,
                                int clip, float* out, double* stats, double* partial, hipStream_t stream);
int hrn_launch_shift_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                   int H, int W, int border, int metric, int clip, float* d_srs, hipStream_t stream);

// ---- cssim.hip: the shift-searched, brightness-corrected SSIM (the definition is in include/hrnet_hip.h), over
// shift_loss.hip's crops and offsets.  window: 0 = 11-tap Gaussian, 1 = 7-tap uniform; H, W >= 2 border + taps.  out [B], stats [B][4] =
// {n*, bias*, score*, k*}, scores [B][(2 border + 1)^2] (may be null).  The callers have checked the arguments.
size_t hrn_shift_cssim_workspace_bytes_impl(int B, int H, int W, int border, int window);
int hrn_launch_shift_cssim(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int window, int clip,
                           int correct_bias, float data_range, float* out, double* stats, double* scores, void* workspace,
                           hipStream_t stream);

// ---- cssim_bwd.hip: the gradient of that score with respect to srs through the offset k* of `stats`, the bias attached (DESIGN.md
// section 7l).  d_srs [B][H][W], every element written.  The callers have checked the arguments.
size_t hrn_cssim_loss_backward_workspace_bytes_impl(int B, int H, int W, int border, int window);
int hrn_launch_cssim_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                   int H, int W, int border, int window, int clip, int correct_bias, float data_range, float* d_srs,
                                   void* workspace, hipStream_t stream);

// ---- cl1_loss.hip: the shift-searched, brightness-corrected L1 / Charbonnier as a training tail (the definition is
// in include/hrnet_hip.h), over shift_loss.hip's crops and offsets, border 0..8.  Forward: a pre-pass for every offset's {n_k, b_k}, a
// main pass for sum m rho(e) and sum m rho'(e), fixed-order finishes -> out [B], stats [B][5] = {n*, b*, cL1*, k*, sigma*} (n* = 0,
// k* = -1, out NaN without a clear pixel).  Backward: d_srs [B][H][W], every element written, through the selected offset only, the bias
// attached.  eps: 0 = |e|, else sqrt(e^2 + eps^2).  The callers have checked the arguments.
size_t hrn_cl1_loss_workspace_bytes_impl(int B, int H, int W, int border);
int hrn_launch_cl1_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, float eps,
                              float* out, double* stats, double* workspace, hipStream_t stream);
int hrn_launch_cl1_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                 int H, int W, int border, int clip, float eps, float* d_srs, hipStream_t stream);

// ---- registration.hip: the masked-NCC sub-pixel registration of LR views (the definitions are in
// include/hrnet_hip.h).  One workgroup per view; a mask pointer may be null (all ones); the callers have checked the limits below.
constexpr int HRN_MNCC_MIN_SIDE = 16, HRN_MNCC_MAX_SIDE = 128;     // a view, its row-pass buffer and its mask patterns fit one CU's LDS
constexpr int HRN_MNCC_MIN_POINTS = 3, HRN_MNCC_MAX_POINTS = 9, HRN_MNCC_MAX_LEVELS = 16;
int hrn_launch_mncc_grid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B,
                         int V, int H, int W, int P, float width, float* scores, hipStream_t stream);
int hrn_launch_mncc_search(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                           int P, int levels, float radius, float* shifts, float* trace, hipStream_t stream);
int hrn_launch_mncc_apply(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                          float* out_valid, hipStream_t stream);

// ---- registration_scene.hip: the same search and resampling for frames of any size, in tiles.  workspace:
// hrn_mncc_scene_workspace_bytes_impl bytes; hrn_mncc_scene_grid_fits: the tiles of all views fit one launch's grid.
constexpr int HRN_MNCC_SCENE_MIN_SIDE = 16, HRN_MNCC_SCENE_MAX_SIDE = 16384;
constexpr int HRN_MNCC_SCENE_TILE = 64;                            // the core tile a workgroup owns, a side
constexpr int HRN_MNCC_SCENE_MEAN_CHUNK = 16384, HRN_MNCC_SCENE_MEAN_CHUNKS = 64;  // a frame's mean: chunks of at least this many pixels, at most so many
size_t hrn_mncc_scene_workspace_bytes_impl(int B, int V, int H, int W, int P);
bool hrn_mncc_scene_grid_fits(int B, int V, int H, int W);
int hrn_launch_mncc_grid_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres,
                               int B, int V, int H, int W, int P, float width, float* scores, void* workspace, hipStream_t stream);
// init: (B,V,2) or null for (0, 0); last_trace / last_stride: where the last level's (dy, dx, score) goes when `trace` is null
int hrn_launch_mncc_search_scene_from(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init,
                                      int B, int V, int H, int W, int P, int levels, float radius, float* shifts, float* trace,
                                      float* last_trace, int last_stride, void* workspace, hipStream_t stream);
int hrn_launch_mncc_apply_scene(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                                float* out_valid, hipStream_t stream);
// the pre-pass of the frames' means, for registration_local.hip as well
void hrn_launch_mncc_scene_means(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H,
                                 int W, double* means, hipStream_t stream);      // means[((plane) * chunks + chunk) * 2] = {sum, count}

// ---- resample_bwd.hip: the backward of hrn_launch_mncc_apply_scene.  d_views or d_shifts may be null: that half
// is not launched; views and the workspace (hrn_mncc_apply_backward_workspace_bytes_impl bytes) are read only for d_shifts.
size_t hrn_mncc_apply_backward_workspace_bytes_impl(int B, int V, int H, int W);
int hrn_launch_mncc_apply_backward(const float* views, const float* shifts, const float* valid, const float* d_out, int B, int V, int H,
                                   int W, float* d_views, float* d_shifts, void* workspace, hipStream_t stream);

// ---- subpixel_loss.hip: the sub-pixel searched cMSE / cPSNR loss (the definition is in include/hrnet_hip.h): the
// scene path's grid search scored by the brightness-corrected cMSE of S(sr, s) against hr, and the gradient through the sampler at the
// point found.  out [B], stats [B][8] = {n*, b*, cMSE*, dy*, dx*, mean sr, mean hr under m0, centred bias}, trace [B][levels][3] or null.
// The two workspaces are apart: the forward's m0 and scene plan, the backward's g, c and fp32 shifts.  The callers have checked the
// arguments.
size_t hrn_subpixel_loss_forward_bytes_impl(int B, int H, int W, int P);
size_t hrn_subpixel_loss_backward_bytes_impl(int B, int H, int W);
int hrn_launch_subpixel_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int P, int levels,
                                   float radius, int metric, float* out, double* stats, float* trace, void* workspace, hipStream_t stream);
int hrn_launch_subpixel_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                      int H, int W, int border, int metric, float* d_srs, void* workspace, hipStream_t stream);

// ---- registration_local.hip: a shift per block of tiles of every view, and the views resampled by the field between the blocks'
// centres.  block: a multiple of 64 in 64..4096; hrn_mncc_local_blocks_impl: the blocks of an axis.
constexpr int HRN_MNCC_LOCAL_MIN_BLOCK = 64, HRN_MNCC_LOCAL_MAX_BLOCK = 4096;
int hrn_mncc_local_blocks_impl(int L, int block);
size_t hrn_mncc_local_workspace_bytes_impl(int B, int V, int H, int W, int P, int block);
bool hrn_mncc_local_grid_fits(int B, int V, int H, int W, int block);
int hrn_launch_mncc_search_local(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init,
                                 int B, int V, int H, int W, int P, int levels, float radius, int block, float min_valid, float* field,
                                 float* trace, float* ok, void* workspace, hipStream_t stream);
int hrn_launch_mncc_apply_field(const float* views, const float* view_masks, const float* field, int B, int V, int H, int W, int block,
                                float* out, float* out_valid, hipStream_t stream);

// ---- registration_pyramid.hip: the masked 2:1 reduction of planes and the coarse-to-fine search over `octaves` of them (DESIGN.md
// section 7j).  reduce2 takes two sets of planes of one size in one launch (nb may be 0); a mask pointer may be null (all clear).
constexpr int HRN_MNCC_REDUCE_MIN_SIDE = 32, HRN_MNCC_MAX_OCTAVES = 6;
constexpr float HRN_MNCC_PYRAMID_MAX_REACH = 128.f;                // radius * 2^octaves, in pixels of the frame
bool hrn_mncc_reduce2_grid_fits(size_t planes, int H, int W);
int hrn_launch_mncc_reduce2(const float* a, const float* a_mask, size_t na, const float* b, const float* b_mask, size_t nb, int H, int W,
                            float* a_out, float* a_out_mask, float* b_out, float* b_out_mask, hipStream_t stream);
size_t hrn_mncc_pyramid_workspace_bytes_impl(int B, int V, int H, int W, int P, int octaves);
int hrn_launch_mncc_search_pyramid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H,
                                   int W, int P, int octaves, int levels, float radius, int coarse_levels, float refine_radius, float* shifts,
                                   float* trace, void* workspace, hipStream_t stream);

// ---- shiftnet.hip.  dt: storage of the activation tensors x / out / y - HRN_F32 or HRN_BF16, one bf16 plane (ShiftNet's bf16
// training mode); statistics, scale / shift and fc1's input xr are f32 in both
int hrn_launch_bn_stats(int dt, const void* x, size_t npix, int C, const float* gamma, const float* beta, float eps,
                        float* scale, float* shift, float* running_mean, float* running_var, float momentum,
                        double* partial, int partial_blocks, hipStream_t stream);
int hrn_launch_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                       const float* conv_bias, float* scale, float* shift, int C, hipStream_t stream);
int hrn_launch_bn_act_pool(int dt, const void* x, const float* scale, const float* shift, void* out, int N, int H, int W, int C,
                           int pool, hipStream_t stream);
// fc1: xr = the input in the reference's flatten order (hrn_launch_fc_to_ref: from the NHWC activation, dropout folded in), w = the raw
// fc1.weight (1024, 32768), partial = hrn_fc1_partial_bytes() of scratch
int hrn_launch_fc_to_ref(int dt, const void* y, const unsigned char* mask, float* xr, int B, hipStream_t stream);
size_t hrn_fc1_partial_bytes(void);
int hrn_launch_fc1(const float* xr, const float* w, const float* b, float* y, int B, float* partial, hipStream_t stream);
int hrn_launch_fc2(const float* y, const float* w, float* theta, int B, hipStream_t stream);
// ---- shiftnet_bwd.hip: the backward's own passes, launchable alone (kernel_test.hip).  dt as above (HRN_F32 or HRN_BF16).
// BatchNorm (+ ReLU, + MaxPool2d(2) when pool) backward of one layer: x = the pre-BatchNorm tensor [N][H][W][C], dy = the gradient of
// the layer's output [N][H/p][W/p][C], stats = {mean, invstd, scale, shift} x 128 floats; writes dx [N][H][W][C], accumulates
// dgamma / dbeta.  partial: SN_PARTIAL_BLOCKS x 128 x 2 doubles, sums: 128 x 2 doubles.
int hrn_launch_sn_bn_bwd(int dt, const void* x, const void* dy, const float* stats, const float* gamma, void* dx, float* dgamma, float* dbeta,
                         int N, int H, int W, int C, int pool, double* partial, double* sums, hipStream_t s);
// the stem's (2 -> 64, ShiftNet.py:17) input gradient: g [M][H][W][64] (dt), w the raw weights (64, 2, 3, 3) -> din [M][2][H][W] f32
int hrn_launch_sn_stem_dgrad(int dt, const void* g, const float* w, float* din, int M, int H, int W, hipStream_t s);
// dy [B][16*16][128] (dt) = the gradient of fc1's input dxr (B, 32768) f32 in the reference's flatten order, dropout mask applied
int hrn_launch_fc_from_ref(int dt, const float* dxr, const unsigned char* mask, void* dy, int B, hipStream_t s);
// mean[c], invstd[c] (what the BatchNorm backward reads) from the `partial` sums hrn_launch_bn_stats left (SN_PARTIAL_BLOCKS of them)
int hrn_launch_sn_bn_save_stats(const double* partial, size_t npix, int C, float eps, float* mean, float* invstd, hipStream_t s);
// out [planes][hw] = g - means[plane]: the backward of the per-plane mean subtraction (ShiftNet.py:58)
int hrn_launch_sn_sub_plane_mean(const float* g, const float* means, float* out, int planes, size_t hw, hipStream_t s);
// the tail's backward, any batch size: dz1 (B, 1024) = (y1 > 0) dtheta w2, dw2 (2, 1024) += dtheta^T y1, db1 (1024) += sum_b dz1 (dw2 /
// db1 NULL: frozen); dw1 (1024, 32768) += dz1^T xr and dxr (B, 32768) = dz1 w1, both in groups of 32 samples (one launch per group)
int hrn_launch_sn_fc2_bwd(const float* dtheta, const float* y1, const float* w2, float* dz1, float* dw2, float* db1, int B, hipStream_t s);
int hrn_launch_sn_fc1_bwd_w(const float* dz1, const float* xr, float* dw1, int B, hipStream_t s);
int hrn_launch_sn_fc1_bwd_x(const float* dz1, const float* w1, float* dxr, int B, hipStream_t s);
