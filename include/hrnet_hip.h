/* hrnet_hip.h - C ABI of libhrnet_hip.so: the MI355X (gfx950) implementation of the HighRes-net hot path.
 *
 * The reference (gwall-ceres/HighRes-net) has no FFI: its boundary is three Python symbols.  Every entry point
 * below replaces one of them (or one stage of one); `highres-net_amd/hrnet_hip/binding.py` binds them with
 * ctypes and `highres-net_amd/{DeepNetworks/HRNet.py,DeepNetworks/ShiftNet.py,lanczos.py}` re-expose the
 * reference's module names on top.
 *
 *   hrn_hrnet_forward      <-  HRNet.forward(lrs, alphas)            src/DeepNetworks/HRNet.py:186-211
 *   hrn_encoder_forward    <-  median/stack + Encoder.forward         src/DeepNetworks/HRNet.py:200-206, :62-74
 *   hrn_fuse_forward       <-  RecuversiveNet.forward                 src/DeepNetworks/HRNet.py:99-134
 *   hrn_decoder_forward    <-  Decoder.forward                        src/DeepNetworks/HRNet.py:158-169
 *   hrn_*_s                <-  the same at upscale factor 2, 3 or 4   src/DeepNetworks/HRNet.py:147-156 (config decoder.deconv)
 *   hrn_shiftnet_forward   <-  ShiftNet.forward(x)                    src/DeepNetworks/ShiftNet.py:49-75
 *   hrn_lanczos_shift      <-  lanczos.lanczos_shift(img, shift, ...) src/lanczos.py:47-107
 *                              (and ShiftNet.transform, ShiftNet.py:77-90, which only re-labels its arguments)
 *   hrn_lanczos_kernel     <-  lanczos.lanczos_kernel(dx, a=3, N=7)   src/lanczos.py:5-43
 *   hrn_*_pack             <-  nn.Module.load_state_dict / .to(device): reference-layout f32 parameters
 *                              (OIHW conv, (Cin,Cout,kH,kW) deconv, (out,in) linear) -> kernel layouts
 *   hrn_hrnet_forward_train / hrn_hrnet_backward, hrn_shiftnet_forward_train / hrn_shiftnet_backward,
 *   hrn_lanczos_shift_backward  <-  torch autograd through the three symbols above, src/train.py:172-190
 *   hrn_adam_step          <-  optimizer.step() of torch.optim.Adam   src/train.py:191, :252
 *   hrn_grad_sumsq / hrn_optim_prepare / hrn_adam_step_ex  <-  (no counterpart: the reference's loop has none of them)
 *                              torch.nn.utils.clip_grad_norm_, a skip of non-finite steps, torch.optim.AdamW and an EMA of the weights
 *   hrn_get_loss / hrn_shift_cpsnr  <-  get_loss (train.py:66-87) / shift_cPSNR (Evaluator.py:52-73)
 *   hrn_shift_loss_train / hrn_shift_loss_backward  <-  the two combined as a differentiable loss (the searched score, trainable)
 *   hrn_shift_cssim / hrn_cssim_loss_backward  <-  (no counterpart: the project's second score) the shift-searched, brightness-corrected
 *                              SSIM, and its gradient through the selected offset: cSSIM as a training loss
 *   hrn_cl1_loss_train / hrn_cl1_loss_backward  <-  (no counterpart: the project's third searched loss) the shift-searched,
 *                              brightness-corrected L1 / Charbonnier, and its gradient through the selected offset
 *   hrn_mncc_grid / hrn_mncc_search / hrn_mncc_apply  <-  the method of the fork's registration_search.py (recursive_mncc_search over
 *                              compute_grid_mncc), restated: sub-pixel registration of the LR views against a reference frame;
 *                              hrn_mncc_grid_scene / hrn_mncc_search_scene / hrn_mncc_apply_scene: the same for frames of any size;
 *                              hrn_mncc_search_local / hrn_mncc_apply_field: a shift per block of a scene and the resampling by that field
 *   hrn_mncc_apply_backward  <-  (no counterpart: the fork's search is never differentiated) the gradient of hrn_mncc_apply_scene with
 *                              respect to the views and to the shifts: the resampler as a differentiable warp
 *   hrn_collate_device     <-  collateFunction(min_L) over ImagesetDataset items (src/utils.py:63-113), gathered from
 *                              imagesets decoded once into HBM (DataLoader.DeviceImagesetCache); hrn_collate_device_s
 *                              is the same for x2 / x3 / x4 targets
 *   hrn_collate_device_a   <-  (no counterpart: the reference trains without augmentation) the same gather with one of the
 *                              eight flips / rotations of the square applied per sample; hrn_collate_device_m also gathers the
 *                              LR quality masks (QM*.png) of the views it picks
 *   hrn_resample_targets   <-  (no counterpart) HR / SM stored at one ratio resampled to another when the cache is built
 *   hrn_dihedral_expand / hrn_dihedral_mean  <-  (no counterpart: the reference predicts from one orientation) the two ends of a
 *                              flip / rotate self-ensemble at inference: the K transformed copies of the view stack, and the mean
 *                              of the K predictions after each is transformed back
 *   hrn_tile_gather / hrn_tile_scatter / hrn_tile_count / hrn_hrnet_halo  <-  (no counterpart in the reference: it predicts
 *                              square chips whole) the two ends of tiled inference: overlapping square windows of a scene of
 *                              any size and aspect ratio, and the windows' cores put back into the scene's prediction
 *   hrn_masked_composite / hrn_hrnet_*_ref  <-  (no counterpart: the reference's frame is the plain median of lrs[:, :9], HRNet.py:200)
 *                              a cloud-free reference frame from the views and their quality masks, and HRNet given that frame
 *   hrn_upsample / hrn_upsample_backward  <-  (no counterpart: the reference's network synthesises the whole image) bicubic x2 / x3 / x4
 *                              interpolation of a frame with an add, and its adjoint: the global residual over an upsampled LR frame
 *   hrn_shift_add / hrn_shift_add_backward  <-  (no counterpart: the reference has no classical multi-frame predictor) shift-and-add of the
 *                              registered views onto the x2 / x3 / x4 grid (normalised convolution), and its adjoint
 *   hrn_observe / hrn_consistency_residual / hrn_consistency_finish / hrn_observe_adjoint  <-  (no counterpart) the observation model: what
 *                              every registered view should have recorded of an HR frame, the data-consistency loss and back-projection
 *   hrn_observe_shift_grad / _grad_finish / hrn_shift_normal / hrn_shift_normal_finish  <-  (no counterpart) the observation model's
 *                              derivative in the shifts: the gradient to a registration, and Gauss-Newton refinement of the shifts
 *   hrn_robust_sums / hrn_robust_finish / hrn_robust_apply / hrn_btv_step / hrn_btv_backward / hrn_btv_value  <-  (no counterpart) Welsch
 *                              weights for the data term and a bilateral-TV prior: the robust, regularised reconstruction
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed or a torch CUDA tensor's data_ptr) unless stated;
 *     all tensors are dense / contiguous; images are square-agnostic here (the Python mirror asserts H == W
 *     where the reference's .view() does, HRNet.py:204);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work: no allocation,
 *     no synchronisation, no host read-back, so a call sequence can be captured into a hipGraph;
 *   - the caller owns every buffer, including the workspace (size from the matching *_workspace_bytes);
 *   - return value: 0 on success, negative on error (-2 bad argument, -3 workspace/packed buffer too small,
 *     -5 HIP runtime error); hrn_last_error() returns a thread-local message for the last failing call;
 *   - dtype selects storage of activations and the MFMA input type:
 *       HRN_DTYPE_F32  : f32 activations, v_mfma_f32_32x32x2_f32 (exact fp32 products and accumulation)
 *       HRN_DTYPE_BF16 : bf16 activations/weights, fp32 accumulation: v_mfma_f32_16x16x32_bf16 in the encoder's 64 -> 64 convs and
 *                        the fusion levels (128 -> {128, 64} convs), v_mfma_f32_32x32x16_bf16 in the stem, the decoder and the
 *                        general conv kernel (the route of images beyond the 32-bit in-image offsets)
 *       HRN_DTYPE_BF16X3 : every fp32 activation / weight as two bf16 planes (hi = bf16(v), lo = bf16(v - hi)); a product is
 *                        hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (~2^-16 per product): the
 *                        reference's fp32 arithmetic (train.py:168-171, predict.py:36-37) to ~1e-5 at a third of the bf16
 *                        matrix rate.  Stage tensors (emb, fused) are [2 planes][...][64] bf16, lo plane directly behind hi.
 *     inputs (lrs, alphas, ShiftNet pairs, Lanczos images) and the SR output are always f32;
 *   - a packed HRNet blob is only valid for the dtype AND the upscale factor (`scale`) it was packed with: the *_s entry points take
 *     the scale explicitly (2, 3 or 4: decoder.deconv kernel_size == stride, src/DeepNetworks/HRNet.py:147-156), the others are
 *     their scale = 3 case (the reference's shipped config).  Any other scale: -2 before any launch, and 0 from the *_bytes_s sizes.
 */
#ifndef HRNET_HIP_H
#define HRNET_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRN_DTYPE_F32 0
#define HRN_DTYPE_BF16 1
#define HRN_DTYPE_BF16X3 2
#define HRN_MAX_RES_LAYERS 8
#define HRN_ABI_VERSION 1
#define HRN_COLLATE_META 5     /* leading int64 fields of a hrn_collate_device plan row */

int hrn_version(void);
const char* hrn_last_error(void);

/* ------------------------------------------------------------------ HRNet */
/* Parameters exactly as the reference's state_dict holds them (f32, contiguous). */
typedef struct hrn_hrnet_params {
    int num_layers;                                   /* config["encoder"]["num_layers"], 0..HRN_MAX_RES_LAYERS */
    const float* enc_init_w;                          /* encode.init_layer.0.weight (64,2,3,3) */
    const float* enc_init_b;                          /* encode.init_layer.0.bias   (64)       */
    const float* enc_init_a;                          /* encode.init_layer.1.weight (1)  PReLU */
    const float* enc_res_w[2 * HRN_MAX_RES_LAYERS];   /* encode.res_layers.L.block.{0,2}.weight (64,64,3,3), index 2L+{0,1} */
    const float* enc_res_b[2 * HRN_MAX_RES_LAYERS];   /* ... .bias (64) */
    const float* enc_res_a[2 * HRN_MAX_RES_LAYERS];   /* encode.res_layers.L.block.{1,3}.weight (1) */
    const float* enc_final_w;                         /* encode.final.0.weight (64,64,3,3) */
    const float* enc_final_b;                         /* encode.final.0.bias */
    const float* fuse_res_w[2];                       /* fuse.fuse.0.block.{0,2}.weight (128,128,3,3) */
    const float* fuse_res_b[2];
    const float* fuse_res_a[2];                       /* fuse.fuse.0.block.{1,3}.weight (1) */
    const float* fuse_out_w;                          /* fuse.fuse.1.weight (64,128,3,3) */
    const float* fuse_out_b;
    const float* fuse_out_a;                          /* fuse.fuse.2.weight (1) */
    const float* dec_w;                               /* decode.deconv.0.weight (64,64,3,3) = (Cin,Cout,kH,kW); (64,64,S,S) at scale S */
    const float* dec_b;
    const float* dec_a;                               /* decode.deconv.1.weight (1) */
    const float* fin_w;                               /* decode.final.weight (1,64,1,1) */
    const float* fin_b;                               /* decode.final.bias (1) */
} hrn_hrnet_params;

size_t hrn_hrnet_packed_bytes(int dtype, int num_layers);
int hrn_hrnet_pack(const hrn_hrnet_params* params, int dtype, void* packed, size_t packed_bytes, void* stream);

size_t hrn_hrnet_workspace_bytes(int dtype, int B, int V, int H, int W);

/* lrs (B,V,H,W) f32, alphas (B,V) f32 -> sr (B,1,3H,3W) f32 */
int hrn_hrnet_forward(const void* packed, int dtype, int num_layers, int alpha_residual,
                      const float* lrs, const float* alphas, int B, int V, int H, int W,
                      float* sr, void* workspace, size_t workspace_bytes, void* stream);

/* Stages (same workspace).  emb: view stack [B][V][H][W][64] in `dtype` (channels-last); fused: [B][H][W][64].
 * HRN_DTYPE_BF16X3: emb is [2][B][V][H][W][64] bf16 and fused [2][B][H][W][64] bf16 (plane 0 = hi, plane 1 = lo). */
int hrn_encoder_forward(const void* packed, int dtype, int num_layers, const float* lrs, int B, int V, int H, int W,
                        void* emb, void* workspace, size_t workspace_bytes, void* stream);
/* Destroys `emb` (levels are reduced in place, HRNet.py:113-132). */
int hrn_fuse_forward(const void* packed, int dtype, int num_layers, int alpha_residual, void* emb, const float* alphas,
                     int B, int V, int H, int W, void* fused, void* workspace, size_t workspace_bytes, void* stream);
int hrn_decoder_forward(const void* packed, int dtype, int num_layers, const void* fused, int N, int H, int W,
                        float* sr, void* stream);

/* Any upscale factor scale in {2, 3, 4} (ConvTranspose2d(64, 64, scale, stride=scale), HRNet.py:147-156).  Only the decoder
 * depends on it: the blob's decoder weights, dec_w (64,64,scale,scale), and the SR size (B,1,scale H,scale W).
 *   hrn_hrnet_packed_bytes_s / hrn_hrnet_pack_s  <-  load_state_dict of a model built with that config (HRNet.py:138-156)
 *   hrn_hrnet_forward_s                          <-  HRNet.forward(lrs, alphas)   HRNet.py:186-211: sr (B,1,scale H,scale W)
 *   hrn_decoder_forward_s                        <-  Decoder.forward              HRNet.py:158-169: sr (N,1,scale H,scale W)
 * The workspace (hrn_hrnet_workspace_bytes) and the encoder / fusion stages above do not depend on the scale. */
size_t hrn_hrnet_packed_bytes_s(int dtype, int num_layers, int scale);
int hrn_hrnet_pack_s(const hrn_hrnet_params* params, int dtype, int scale, void* packed, size_t packed_bytes, void* stream);
int hrn_hrnet_forward_s(const void* packed, int dtype, int num_layers, int scale, int alpha_residual,
                        const float* lrs, const float* alphas, int B, int V, int H, int W,
                        float* sr, void* workspace, size_t workspace_bytes, void* stream);
int hrn_decoder_forward_s(const void* packed, int dtype, int num_layers, int scale, const void* fused, int N, int H, int W,
                          float* sr, void* stream);

/* Training path (fp32; bf16x3 and bf16 through the _dt / _s / _in forms below): `srs = fusion_model(lrs, alphas)` with grad enabled and `loss.backward()` through HRNet,
 * src/train.py:172-190.  hrn_hrnet_forward_train is hrn_hrnet_forward(HRN_DTYPE_F32) with every intermediate kept in
 * `train_ws`; hrn_hrnet_backward consumes that workspace (same B, V, H, W) and d_sr = dLoss/d sr (B,1,3H,3W) and
 * ACCUMULATES (+=, like autograd's .grad) the parameter gradients into the buffers `grads` points at - the same struct,
 * fields aliasing f32 gradient tensors of the parameters' shapes (the inputs lrs / alphas get no gradient, as in
 * train.py).  `packed` is the HRN_DTYPE_F32 blob of hrn_hrnet_pack, `params` the raw reference-layout tensors.
 * Any PReLU slope is accepted, as in the reference: with a positive slope the backward works from the stored post-activations;
 * behind a slope <= 0 it recomputes the pre-activation (decided on the device: the extra launches exit at once otherwise). */
size_t hrn_hrnet_train_workspace_bytes(int num_layers, int B, int V, int H, int W);
int hrn_hrnet_forward_train(const void* packed, int num_layers, int alpha_residual, const float* lrs, const float* alphas,
                            int B, int V, int H, int W, float* sr, void* train_ws, size_t train_ws_bytes, void* stream);
int hrn_hrnet_backward(const void* packed, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                       const float* alphas, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* grads,
                       void* train_ws, size_t train_ws_bytes, void* stream);
/* The same with a dtype: HRN_DTYPE_F32 (what the two entry points above run); HRN_DTYPE_BF16X3 - every activation and gradient
 * tensor of the workspace a pair of bf16 planes, three bf16 MFMAs per product in the convolutions, their data gradients and their
 * weight gradients; or HRN_DTYPE_BF16 - every activation and gradient tensor of the workspace ONE bf16 plane (stores round to nearest
 * even), one bf16 MFMA per product with fp32 accumulation, reductions (bias, slope, alpha, input-gradient sums) in fp32 / f64 as in
 * the other modes.  `packed` is the blob of that dtype; the workspace size is the same for every dtype (bf16 uses less of it).
 * Parameters, parameter gradients, lrs, alphas, sr, d_sr, d_lrs, d_alphas: f32 in every mode.  In every dtype `packed` and `train_ws`
 * must be 256-byte aligned (as any hipMalloc'd block is); otherwise -2 before any launch. */
int hrn_hrnet_forward_train_dt(const void* packed, int dtype, int num_layers, int alpha_residual, const float* lrs,
                               const float* alphas, int B, int V, int H, int W, float* sr, void* train_ws, size_t train_ws_bytes,
                               void* stream);
int hrn_hrnet_backward_dt(const void* packed, int dtype, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                          const float* alphas, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* grads,
                          void* train_ws, size_t train_ws_bytes, void* stream);
/* The same at any upscale factor scale in {2, 3, 4} (the _dt forms are scale = 3): sr and d_sr are (B,1,scale H,scale W), `packed` is
 * the blob of hrn_hrnet_pack_s at that scale and grads->dec_w (64,64,scale,scale).  `srs = fusion_model(lrs, alphas)` ...
 * `loss.backward()` through HRNet, src/train.py:172-190, for a model whose decoder.deconv has kernel_size == stride == scale.
 * hrn_hrnet_train_workspace_bytes serves every scale (the decoder's scratch at scale 4 is below the convolutions'). */
int hrn_hrnet_forward_train_s(const void* packed, int dtype, int num_layers, int scale, int alpha_residual, const float* lrs,
                              const float* alphas, int B, int V, int H, int W, float* sr, void* train_ws, size_t train_ws_bytes,
                              void* stream);
int hrn_hrnet_backward_s(const void* packed, int dtype, int scale, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                         const float* alphas, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* grads,
                         void* train_ws, size_t train_ws_bytes, void* stream);
/* hrn_hrnet_backward_s that also returns the gradients of the inputs, as torch autograd does through the reference's HRNet
 * (HRNet.py:198-204 for lrs, :113-132 for alphas).  d_lrs (B,V,H,W) f32: the stem's input gradient; its first channel goes to each
 * view, its second (the reference frame, `torch.median(lrs[:, :9], 1)`, HRNet.py:200) is summed over the sample's views and added to
 * ONE view per pixel: the lowest-indexed of the first min(V, 9) views whose value equals the median (where several are tied, torch
 * leaves the choice open).  d_alphas (B,V) f32: at each fusion level d alphas_bob = sum over channels and pixels of
 * dLoss/d x_new * fuse(...) (HRNet.py:124-128); 0 for views that are never bob, and 0 everywhere without the alpha residual.
 * Either pointer may be NULL, which skips that output; input gradients are WRITTEN, parameter gradients still accumulate.
 * hrn_hrnet_backward_s is the NULL / NULL case.  Same workspace, no more bytes of it. */
int hrn_hrnet_backward_in(const void* packed, int dtype, int scale, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                          const float* alphas, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* grads,
                          float* d_lrs, float* d_alphas, void* train_ws, size_t train_ws_bytes, void* stream);
/* hrn_hrnet_backward_in for a partly frozen model (`requires_grad_(False)` on some parameters, src/train.py:172-190): a NULL field of
 * `grads` means "not requested" (`grads` itself must not be NULL), and only the work some requested output depends on is launched.
 * Decoder parameters need the decoder's weight-gradient part alone; any fusion parameter (shared by every level), or d_alphas with the
 * alpha residual, the data gradients of the decoder and of the fusion levels; encoder / stem parameters or d_lrs the chain down to the
 * stem.  Every requested gradient, d_lrs and d_alphas is bit-identical to what hrn_hrnet_backward_in gives with every field set, which
 * is also what this entry point runs then.  Same arguments, checks, workspace and return codes as hrn_hrnet_backward_in.  The other
 * hrn_hrnet_backward* forms are this function with arguments fixed, so they treat a NULL field of `grads` the same way. */
int hrn_hrnet_backward_sel(const void* packed, int dtype, int scale, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                           const float* alphas, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* grads,
                           float* d_lrs, float* d_alphas, void* train_ws, size_t train_ws_bytes, void* stream);

/* ------------------------------------------------------------------ cloud-free composite reference frame
 * (No counterpart in the reference, whose HRNet.py:200 takes the plain lower median of lrs[:, :9], clouds, concealed pixels and the
 * zeros of registered views included.)
 *
 * hrn_masked_composite: views (B,V,H,W) f32, masks (B,V,H,W) f32 or NULL (all clear), alphas (B,V) f32 or NULL (every view real)
 * -> ref (B,H,W), count (B,H,W) or NULL, filled (B,V,H,W) or NULL.  Per sample b and pixel p, with n = min(V, n_ref), 1 <= n_ref <= 32:
 *   - a view v < n is REAL when alphas is NULL or alphas[b,v] != 0, and a CANDIDATE when it is real and masks is NULL or masks[b,v,p] != 0;
 *   - with c >= 1 candidates ref[b,p] is their LOWER median - the element at index (c - 1) / 2 in ascending order, the rule of the
 *     network's own reference frame - and count[b,p] = c;
 *   - with c == 0, ref is the lower median over the real views v < n, masks ignored, and count = 0; with no real view either it is the
 *     lower median over all n views, which is the network's own reference frame;
 *   - filled[b,v,p] = views[b,v,p] where view v is not real (padding stays as it is), or masks is NULL, or masks[b,v,p] != 0; otherwise
 *     ref[b,p].  This covers all V views, not only the first n.
 * The inputs must be finite (+inf is the padding key of the selection).  The result is always one of the input values, so it is exact;
 * it is bit-reproducible and a sample does not depend on its batch.  With masks == NULL, alphas == NULL and n_ref == 9, `ref` is the
 * reference frame hrn_hrnet_forward computes, bit for bit.  One launch; views and masks are read once; `filled` must not alias `views`.
 * -2 before any launch for NULL views / ref, n_ref outside 1..32, non-positive sizes, or a batch beyond one launch's grid. */
int hrn_masked_composite(const float* views, const float* masks, const float* alphas, int B, int V, int H, int W, int n_ref, float* ref,
                         float* count, float* filled, void* stream);

/* HRNet with the reference frame given: `ref` (B,H,W) f32 takes the place of the median of lrs[:, :9] as the second input channel of
 * every view (HRNet.py:200-204); everything after it is the same kernels in the same order, and the median is not launched.  With ref
 * equal to that median the results are bit-identical to the plain entry points'.
 *   hrn_hrnet_forward_ref         hrn_hrnet_forward_s plus ref
 *   hrn_hrnet_forward_train_ref   hrn_hrnet_forward_train_s plus ref (read in place: it must stay unchanged until the backward)
 *   hrn_hrnet_backward_ref        hrn_hrnet_backward_sel plus ref (the frame the forward was given) and d_ref (B,H,W) f32 or NULL.
 *                                 d_lrs is the stem's input gradient of channel 0 alone; d_ref is channel 1 summed over the sample's
 *                                 views in view order, WRITTEN like the other input gradients.  The frame is data: nothing is routed
 *                                 back into the views it was made from.
 * A NULL ref is refused with -2; otherwise arguments, checks, workspaces and return codes are those of the forms they extend. */
int hrn_hrnet_forward_ref(const void* packed, int dtype, int num_layers, int scale, int alpha_residual, const float* lrs,
                          const float* alphas, const float* ref, int B, int V, int H, int W, float* sr, void* workspace,
                          size_t workspace_bytes, void* stream);
int hrn_hrnet_forward_train_ref(const void* packed, int dtype, int num_layers, int scale, int alpha_residual, const float* lrs,
                                const float* alphas, const float* ref, int B, int V, int H, int W, float* sr, void* train_ws,
                                size_t train_ws_bytes, void* stream);
int hrn_hrnet_backward_ref(const void* packed, int dtype, int scale, const hrn_hrnet_params* params, int alpha_residual, const float* lrs,
                           const float* alphas, const float* ref, int B, int V, int H, int W, const float* d_sr,
                           const hrn_hrnet_params* grads, float* d_lrs, float* d_alphas, float* d_ref, void* train_ws, size_t train_ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------ bicubic upsampling and the global residual
 * (No counterpart in the reference, whose network synthesises the whole image; DeepSUM, RAMS and their successors predict the
 * difference to an upsampled LR frame.  HRNet's `global_residual` adds up(frame) to the decoder's output with hrn_upsample.)
 *
 * hrn_upsample: frames (n_planes,H,W) f32, base (n_planes,SH,SW) f32 or NULL -> out[n] = (base ? base[n] : 0) + up(frames[n]),
 * (n_planes,SH,SW), for an integer scale S in {2, 3, 4}.  up() is the bicubic interpolation of
 * torch.nn.functional.interpolate(mode="bicubic", align_corners=False) with Keys' parameter a (-0.75: torch and OpenCV; -0.5: Keys and
 * Pillow).  Output row j has the source coordinate x_j = (j + 0.5) / S - 0.5, i = floor(x_j), t = x_j - i; its four taps sit on the rows
 * i - 1 .. i + 2, the INDICES CLAMPED to 0 .. H - 1, with the weights w2(t + 1), w1(t), w1(1 - t), w2(2 - t),
 *     w1(x) = ((a + 2) x - (a + 3)) x^2 + 1,    w2(x) = ((a x - 5 a) x + 8 a) x - 4 a.
 * Columns likewise; the 2-D filter is the separable product.  An axis has only S phases t: the S x 4 weights are computed on the host in
 * fp64, rounded to fp32 and handed to the kernel by value.  Every phase's weights sum to 1.  The sum is formed in fp32 in one fixed order:
 * the column taps first (w0 f0, then one fma per tap, taps ascending), then the row taps over those sums in the same way, then the add
 * of base.  base may be out itself (the in-place add); frames must not overlap out.  One launch for any n_planes.
 *
 * hrn_upsample_backward WRITES d_frames (n_planes,H,W) = up^T(d_out), the adjoint as a gather: an LR pixel sums the output-gradient
 * pixels whose taps reach it, a border pixel also what the clamped rows and columns beyond the edge collect (with H or W below 3 several
 * fold onto one).  No atomics, one fixed order, bit-reproducible; a plane's result does not depend on its batch, in either function.
 * The gradient with respect to base is d_out itself.
 *
 * Planes of 1 .. 16384 a side, any aspect ratio; every plane and row offset is 64-bit.  -2 before any launch for NULL frames / out /
 * d_out / d_frames, a scale outside {2, 3, 4}, a non-finite a, non-positive sizes, a side beyond 16384, frames overlapping out, a base
 * that overlaps out without being out, or d_frames overlapping d_out.  A workgroup owns HRN_UPSAMPLE_TILE_H x HRN_UPSAMPLE_TILE_W LR pixels. */
#define HRN_UPSAMPLE_TILE_H 8
#define HRN_UPSAMPLE_TILE_W 32
int hrn_upsample(const float* frames, const float* base, float* out, int64_t n_planes, int H, int W, int scale, float a, void* stream);
int hrn_upsample_backward(const float* d_out, float* d_frames, int64_t n_planes, int H, int W, int scale, float a, void* stream);

/* ------------------------------------------------------------------ shift-and-add (normalised convolution)
 * (No counterpart in the reference.)  Every clear LR sample of every registered view is placed at its sub-pixel position on the HR grid,
 * and an HR pixel is the weighted mean of the samples near it, blended with an optional base frame.
 *
 * views, view_masks (B,V,H,W) f32; a mask is 0 / non-zero, view_masks NULL = all ones.  alphas (B,V) or NULL; a view counts iff its alpha
 * is non-zero (a flag, not a weight).  shifts (B,V,2) f32 = (dy, dx) in the registration convention Registered(y,x) = View(y+dy, x+dx):
 * reference coordinate y lies at view coordinate y + dy, so what the masked-NCC searches return goes in unchanged.  scale S in {2, 3, 4}.
 *   HR grid: HR row Y = S m + p has the reference coordinate y = m + t_p, t_p = (p + 0.5) / S - 0.5 (the upsampler's grid).
 *   Taps, per axis and view: d = t_p + dy, formed in fp64 from the fp32 shift, rounded to fp32; at or beyond +-256 it is taken as +-256.
 *     A view with a non-finite shift contributes nothing.  n = floor(d), f = d - n in fp64 (exact); four taps o = -1 .. 2, tap o reads view
 *     row m + n + o at distance u = o - f with the weight
 *         k(u) = exp(-u^2 / (2 sigma^2)) cos^2(pi u / 4)  for |u| < 2,  else 0,
 *     which is non-negative and vanishes with zero slope at the ends of its support: a floor that falls the other way moves nothing, and
 *     the result is C^1 in the shift.  The S x 4 weights of an axis of a view are formed in fp64 (u from the fp32 d, sigma from its fp32
 *     value) and rounded to fp32; a weight below 2^-60 is taken as 0, so that every product k_y k_x that enters a sum is a normal fp32
 *     number (no term of D underflows, and D is either exactly 0 or at least 2^-120).  sigma is in LR pixels, in [0.1, 1].  Columns likewise; a sample's weight is the product k_y k_x.
 *   Sums: N(Y,X) = sum over v, o_y, o_x of k_y k_x x, D(Y,X) the same without x.  A tap outside the frame, a masked sample and a view that
 *     does not count contribute nothing (there is no padding rule).  fp32: per view the column taps first, then the row taps over those
 *     sums (slots ascending, one fma each), added to N and D with the views in index order.
 *   Output: out = (N + prior b) / (D + prior) where D + prior >= 2^-20, else b; b = base (B,SH,SW), 0 when base is NULL; prior >= 0 is the
 *     weight of the base in units where one sample at distance 0 weighs 1.  weight (B,SH,SW) = D is a second output and may be NULL.
 *     base may be out itself; nothing else may overlap an output.
 * hrn_shift_add_backward: out is linear in views and base, D depends on masks and shifts only.  It takes the forward's `weight` (D) and,
 * with q = d_out / (D + prior) where D + prior >= 2^-20, else 0, WRITES
 *     d_views(v,i,j) = [v counts][(i,j) clear] * sum over the HR pixels whose taps reach (i,j) of k_y k_x q   (a gather over at most
 *                      (4 S)^2 HR pixels, no atomics),
 *     d_base = prior q, or d_out where the fallback holds.
 * Either of d_views / d_base may be NULL, and then that half does not run.  There is no gradient to shifts, masks or alphas.
 * Both functions are bit-reproducible, a sample's result does not depend on its batch, and appended views with alpha 0 change no bit.
 * H, W in 1 .. 16384, any B, V >= 1; every offset is 64-bit.  -2 before any launch for a NULL views / shifts / out / d_out / weight (of the
 * backward), non-positive sizes, a side beyond 16384, a scale outside {2, 3, 4}, a sigma outside [0.1, 1] or a prior below 0 (or either not
 * finite), or overlapping arguments.  A workgroup owns HRN_SHIFT_ADD_TILE_H x HRN_SHIFT_ADD_TILE_W LR pixels. */
#define HRN_SHIFT_ADD_TILE_H 8
#define HRN_SHIFT_ADD_TILE_W 32
int hrn_shift_add(const float* views, const float* view_masks, const float* alphas, const float* shifts, const float* base, float* out,
                  float* weight, int B, int V, int H, int W, int scale, float sigma, float prior, void* stream);
int hrn_shift_add_backward(const float* d_out, const float* weight, const float* view_masks, const float* alphas, const float* shifts,
                           float* d_views, float* d_base, int B, int V, int H, int W, int scale, float sigma, float prior, void* stream);

/* ------------------------------------------------------------------ the observation model: A_v, its adjoint, the consistency loss
 * (No counterpart in the reference.)  A_v x is what view v should have recorded of the HR frame x at its registered sub-pixel position.
 *
 * hr (B,SH,SW) f32 with SH = S H, SW = S W exactly, S = scale in {2, 3, 4}; lrs, lr_masks, residual, views, valid (B,V,H,W) f32; a mask is
 * 0 / non-zero, lr_masks NULL = all ones; alphas (B,V) or NULL, a view counts iff its alpha is non-zero (a flag) and both components of its
 * shift are finite.  shifts (B,V,2) f32 = (dy, dx), Registered(y,x) = View(y+dy, x+dx): what the masked-NCC searches return goes in
 * unchanged.  HR row Y lies at the reference coordinate (Y + 0.5) / S - 0.5.
 *   Operator: view sample i integrates the HR frame over one LR pixel, as S point samples per axis at the HR coordinates S (i - dy) + k,
 *     k = 0 .. S - 1, each read with the six-tap sampler of the registration code, t_o(f) = sinc(o - f) sinc((o - f) / 3), o = -2 .. 3,
 *     normalised to sum 1, and averaged.  Per axis and view: c = -S dy, formed in fp64 from the fp32 shift, rounded to fp32, clamped to
 *     +-256; n = floor(c), f = c - n (exact in fp64).  The S samples share f, so there is ONE vector of S + 5 weights,
 *         w_j = (1 / S) sum_{k=0}^{S-1} t_{j-2-k}(f),  t zero outside -2 .. 3,  j = 0 .. S + 4,
 *     formed in fp64 and rounded to fp32 once; it acts on the HR rows S i + n - 2 + j and sums to 1.  Columns likewise; the operator is a
 *     separable (S + 5)-tap filter, the same for every sample of a view, and a decimation by S at an integer offset.  fp32: the row pass
 *     (along x) first, then the column pass, j ascending, one fma each.
 *   No padding rule: sample i is valid iff 0 <= S i + n - 2 and S i + n + S + 2 <= S H - 1, on both axes, at f = 0 too.  One rule is added
 *     to that: a view whose unclamped |c| reaches 256 on an axis (a shift of 256 / S LR pixels or more) has no valid sample at all, since
 *     the clamped coordinate is no longer the view's.
 *   counted = valid and mask != 0 and the view counts.
 *   Adjoint: (A_v^T r)(Y) = sum_i w_{Y - S i - n + 2} r(i) over the at most 4 / 3 / 3 (x2 / x3 / x4) view rows per axis that reach Y: a
 *     gather, no atomics.
 *   Loss, per sample b: e = A_v x - y_v; n_v = sum counted; beta_v = -sum counted e / n_v with `brightness`, else 0 (and 0 when n_v = 0);
 *     r_v = counted (e + beta_v); L_b = sum_v sum r_v^2 / sum_v n_v, exactly 0 when nothing counts; dL_b/dx = (2 / sum n_v) sum_v A_v^T r_v.
 *   Back-projection: x' = x - step (S^2 / V_b) sum_v A_v^T r_v(x), V_b the number of views with n_v > 0 (x' = x when V_b = 0), step in (0, 2).
 *
 * hrn_observe WRITES views = A_v hr where valid and 0 elsewhere, and valid 0 / 1 (there are no masks or alphas here: a view with a
 *   non-finite shift is 0 and nowhere valid).
 * hrn_consistency_residual WRITES residual = e where counted, exact 0 elsewhere, and per tile of HRN_OBSERVE_TILE_H x HRN_OBSERVE_TILE_W
 *   samples the fp64 sums n, sum e, sum e^2 into `workspace` (hrn_observe_workspace_bytes(B, V, H, W) bytes, 8-byte aligned; 0 for sizes
 *   the functions refuse).
 * hrn_consistency_finish adds the tiles' partials of every view in a fixed order (fp64) and WRITES beta (B,V) f32, count (B,V) int32 = n_v,
 *   ssr (B,V) fp64 = sum r_v^2, loss (B) f32 = L_b, n_views (B) int32 = V_b, coef_loss (B) f32 = 2 / sum_v n_v (0 when nothing counts) and
 *   coef_step (B) f32 = step S^2 / V_b (0 when V_b = 0).  Nothing returns to the host.
 * hrn_observe_adjoint: G = sum_v A_v^T [counted] (residual_v + beta_v), counted re-derived from shifts, lr_masks and alphas, the views in
 *   index order; with c_b = coef[b] gain[b] (either NULL = 1) it WRITES out = c_b G when x is NULL, else out = x - c_b G, where x may be out
 *   itself.  beta NULL = 0.  The loss' gradient is (residual, beta, coef_loss, gain = dL), one back-projection step (residual, beta,
 *   coef_step, NULL, x), the adjoint of hrn_observe (the incoming gradient as residual and nothing else).
 * All four are bit-reproducible (one writer per element, fixed orders, no atomics), a sample's result does not depend on its batch, and
 * appended views with alpha 0 change no bit.  H, W in 1 .. 16384, any B, V >= 1; every offset is 64-bit.  -2 before any launch for a NULL
 * required pointer, non-positive sizes, a side beyond 16384, a scale outside {2, 3, 4}, a step outside (0, 2), a workspace that is too
 * small or misaligned, or overlapping arguments (only x may be out). */
#define HRN_OBSERVE_TILE_H 8
#define HRN_OBSERVE_TILE_W 32
size_t hrn_observe_workspace_bytes(int B, int V, int H, int W);
int hrn_observe(const float* hr, const float* shifts, float* views, float* valid, int B, int V, int H, int W, int scale, void* stream);
int hrn_consistency_residual(const float* hr, const float* lrs, const float* lr_masks, const float* alphas, const float* shifts,
                             float* residual, void* workspace, size_t workspace_bytes, int B, int V, int H, int W, int scale, void* stream);
int hrn_consistency_finish(const void* workspace, size_t workspace_bytes, float* beta, int* count, void* ssr, float* loss, int* n_views,
                           float* coef_loss, float* coef_step, int B, int V, int H, int W, int scale, float step, int brightness,
                           void* stream);
int hrn_observe_adjoint(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta,
                        const float* coef, const float* gain, const float* x, float* out, int B, int V, int H, int W, int scale,
                        void* stream);

/* ------------------------------------------------------------------ the observation model's derivative in the shifts
 * (No counterpart in the reference)  Tensors, c, n, f, w_j, `valid`, `counted` are the observation model's, above.
 *
 *   Derivative weights: omega_j = dw_j / dd = -sum_{k=0}^{S-1} k'_{j-2-k}(f) (c = -S d: the factor S cancels the box mean's 1 / S), with
 *     k'_o = (u'_o - k_o sum u') / sum u the derivative tap of the six-tap sampler, u_o = sinc(o - f) sinc((o - f) / 3), u'_o = du_o / df,
 *     sinc' by the series pi (-z / 3 + z^3 / 30 - z^5 / 840), z = pi t, below |t| = 1e-2 (hrn_mncc_apply_backward's k').  omega is formed
 *     in fp64 and rounded to fp32 once, as w is; sum_j omega_j = 0.
 *   Derivative images, for a valid sample: D_y = (omega^y (x) w^x) x and D_x = (w^y (x) omega^x) x on the (S + 5)^2 footprint of A x; fp32,
 *     the row pass first, j ascending, one fma each.  D = 0 - and the matching component of d_shifts exactly 0 - for a view that does not
 *     count, has a non-finite shift or an unclamped |c| >= 256.  The counted set is piecewise constant in the shift: not differentiated.
 *   Gradient: d_shifts[b,v,a] = coef[b] gain[b] sum_i [counted] (g_i + beta_v) D_a,i, the bracket a select, the product and the sums fp64,
 *     rounded to fp32 once.  observe's backward: g = the incoming gradient, no masks, alphas, beta, coef or gain.  The consistency loss':
 *     g = hrn_consistency_residual's residual with hrn_consistency_finish's beta and coef_loss, gain = dL (the derivative of beta_v drops
 *     out because sum r = 0; without `brightness` beta is 0 and the formula the same).
 *   Normal equations of a view: e = A x - y where counted; p = counted, or with beta_prev (B,V) given the Welsch weight
 *     counted exp(-((e + beta_prev) / delta)^2) of hrn_robust_sums.  From the ten fp64 sums P = sum p, sum p e, sum p e^2, sum p D_a,
 *     sum p e D_a, sum p D_a D_b: beta = -sum p e / P with `brightness` (0 without, and 0 when P < 2^-60), m_a = sum p D_a / P with
 *     `brightness` (else 0; D'_a = D_a - m_a projects the bias out),
 *         g_a = sum p (e + beta) D'_a,   H_ab = sum p D'_a D'_b,   q = sum p (e + beta)^2,
 *     normal (B,V,8) fp64 = [P, g_y, g_x, H_yy, H_yx, H_xx, beta, q].
 *   Update (Levenberg-damped Gauss-Newton, fp64): lam = damping (H_yy + H_xx) / 2, step = -(H + lam I)^-1 g, scaled so that its largest
 *     component is at most max_step in magnitude, shifts_out = fp32(shifts + step).  A view keeps its shift's BITS when fixed[b,v] is
 *     non-zero (fixed NULL: none), when it does not count (alpha 0, a non-finite shift, |c| >= 256), when P < 3 (three pixels of full
 *     weight; a Welsch weight is at most 1, so in that mode three inliers' worth), or when the damped determinant or the step is not
 *     positive and finite.
 *
 * hrn_observe_shift_grad WRITES per tile of HRN_OBSERVE_TILE_H x HRN_OBSERVE_TILE_W samples the two sums into `workspace`
 *   (hrn_observe_shift_workspace_bytes(B, V, H, W) bytes = HRN_SHIFT_NORMAL_SUMS doubles per tile, 8-byte aligned; 0 for sizes the functions
 *   refuse); hrn_observe_shift_grad_finish adds a view's tiles in index order and WRITES d_shifts (B,V,2) f32.
 * hrn_shift_normal WRITES the ten sums per tile, with `residual` non-NULL the residual plane with the bits of
 *   hrn_consistency_residual, and with `plain_workspace` non-NULL (hrn_observe_workspace_bytes(B, V, H, W) bytes, 8-byte aligned) that
 *   function's three plain sums n, sum e, sum e^2 per tile with its bits - in both modes - so that hrn_consistency_finish runs on them
 *   unchanged and an iteration that updates the shifts needs no second pass over the frame; hrn_shift_normal_finish WRITES normal and, with shifts_out non-NULL, the updated shifts (shifts_out must not
 *   alias shifts: the adjoint may still run on the old ones).
 * All are bit-reproducible (fixed orders, no atomics), a sample's result does not depend on its batch, appended views with alpha 0 change no
 * bit.  H, W in 1 .. 16384, any B, V >= 1; every offset is 64-bit.  -2 before any launch for a NULL required pointer, non-positive sizes, a
 * side beyond 16384, a scale outside {2, 3, 4}, a delta that is not positive (with beta_prev), a negative or non-finite damping, a max_step
 * that is not positive and finite, a workspace that is too small or misaligned, or overlapping arguments. */
#define HRN_SHIFT_NORMAL_SUMS 10
size_t hrn_observe_shift_workspace_bytes(int B, int V, int H, int W);
int hrn_observe_shift_grad(const float* hr, const float* g, const float* lr_masks, const float* alphas, const float* shifts,
                           const float* beta, void* workspace, size_t workspace_bytes, int B, int V, int H, int W, int scale, void* stream);
int hrn_observe_shift_grad_finish(const void* workspace, size_t workspace_bytes, const float* coef, const float* gain, float* d_shifts,
                                  int B, int V, int H, int W, void* stream);
int hrn_shift_normal(const float* hr, const float* lrs, const float* lr_masks, const float* alphas, const float* shifts,
                     const float* beta_prev, float delta, float* residual, void* plain_workspace, size_t plain_workspace_bytes,
                     void* workspace, size_t workspace_bytes, int B, int V, int H, int W, int scale, void* stream);
int hrn_shift_normal_finish(const void* workspace, size_t workspace_bytes, const float* alphas, const float* shifts,
                            const unsigned char* fixed, void* normal, float* shifts_out, int B, int V, int H, int W, int scale,
                            int brightness, float damping, float max_step, void* stream);

/* ------------------------------------------------------------------ a robust data term and a bilateral-TV prior for the reconstruction
 * (No counterpart in the reference)  Tensors, `counted`, n_v and V_b are the observation model's, above.
 *
 * Robust data step (Welsch weights), per sample and iteration, from the residual e that hrn_consistency_residual wrote and a state
 * beta_prev (B,V) - the plain mean bias of the first iteration (hrn_consistency_finish's beta), afterwards the previous beta:
 *     w = counted exp(-((e + beta_prev) / delta)^2)        (fp32: the sum, the quotient, the square, expf)
 *     beta_v = -sum w e / sum w, 0 when sum w < 2^-60 and 0 without `brightness`;   r' = w (e + beta_v)
 *     x' = x - step (S^2 / V_b) sum_v A_v^T r'_v           (hrn_observe_adjoint on r' with beta = NULL and hrn_consistency_finish's coef_step)
 * hrn_robust_sums WRITES per tile of HRN_OBSERVE_TILE_H x HRN_OBSERVE_TILE_W samples the fp64 sums of w, w e and w (e + beta_prev)^2 (the
 *   products in fp64 of the fp32 w and e) into `workspace` (hrn_robust_workspace_bytes(B, V, H, W) bytes, 8-byte aligned).
 * hrn_robust_finish adds them in a fixed order and WRITES beta (B,V), inlier (B,V) = sum w / n_v (0 when n_v = 0; count is
 *   hrn_consistency_finish's) and loss (B) = sum_v sum w (e + beta_prev)^2 / sum_v sum w (0 when that is below 2^-60).
 * hrn_robust_apply WRITES weighted (B,V,H,W) = r' where counted and exact 0 elsewhere; it must not alias the residual.
 *
 * Bilateral TV of a plane x (SH, SW), P in 1 .. HRN_BTV_MAX_P, 0 < alpha <= 1, eps > 0:
 *     R(x) = sum_{(l,m) != (0,0), |l|,|m| <= P} alpha^(|l|+|m|) sum_p phi(x_p - x_{p-(l,m)}),  phi(t) = sqrt(t^2 + eps^2) - eps,
 *   the inner sum over the pixels whose partner lies inside the plane (no padding; every unordered pair appears twice), and
 *     g_p = dR/dx_p = 2 sum_q alpha^(|l|+|m|) phi'(x_p - x_q),  phi'(t) = t / sqrt(t^2 + eps^2),
 *   over the neighbours q = p + (l, m) inside the plane, in raster order of (l, m), one fma each.  The weights alpha^k are formed in fp64
 *   and rounded to fp32 once; phi' is t rsqrt(fma(t, t, eps^2)), exactly 0 for equal neighbours.
 * hrn_btv_step WRITES out = x - c[plane] g; hrn_btv_backward WRITES out = gain[plane] g.  out must not overlap x (a stencil).
 * hrn_btv_value WRITES value (planes) f32 = gain R / (SH SW) from per-tile fp64 partials (`workspace`: hrn_btv_workspace_bytes bytes,
 *   8-byte aligned), tiles of HRN_BTV_TILE_H x HRN_BTV_TILE_W pixels, added in a fixed order by a second launch.
 * All are bit-reproducible and a plane's or sample's result does not depend on its batch; appended views with alpha 0 change no bit.
 * Sides of 1 .. HRN_BTV_MAX_SIDE for the planes; every offset is 64-bit.  -2 before any launch for a NULL pointer, non-positive or too
 * large sizes, a bad scale, delta, P, alpha, eps or gain, a workspace that is too small or misaligned, or overlapping arguments. */
#define HRN_BTV_TILE_H 16
#define HRN_BTV_TILE_W 64
#define HRN_BTV_MAX_P 3
#define HRN_BTV_MAX_SIDE 49152
size_t hrn_robust_workspace_bytes(int B, int V, int H, int W);
int hrn_robust_sums(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta_prev,
                    void* workspace, size_t workspace_bytes, int B, int V, int H, int W, int scale, float delta, void* stream);
int hrn_robust_finish(const void* workspace, size_t workspace_bytes, const int* count, float* beta, float* inlier, float* loss, int B, int V,
                      int H, int W, int brightness, void* stream);
int hrn_robust_apply(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta_prev,
                     const float* beta, float* weighted, int B, int V, int H, int W, int scale, float delta, void* stream);
int hrn_btv_step(const float* x, const float* c, float* out, int planes, int SH, int SW, int P, float alpha, float eps, void* stream);
int hrn_btv_backward(const float* x, const float* gain, float* out, int planes, int SH, int SW, int P, float alpha, float eps, void* stream);
size_t hrn_btv_workspace_bytes(int planes, int SH, int SW);
int hrn_btv_value(const float* x, float* value, void* workspace, size_t workspace_bytes, int planes, int SH, int SW, int P, float alpha,
                  float eps, float gain, void* stream);

/* ------------------------------------------------------------------ ShiftNet */
typedef struct hrn_shiftnet_params {
    const float* conv_w[8];       /* layerN.0.weight  (co,ci,3,3): 2->64,64->64 x3,64->128,128->128 x3 */
    const float* conv_b[8];       /* layerN.0.bias */
    const float* bn_g[8];         /* layerN.1.weight */
    const float* bn_b[8];         /* layerN.1.bias */
    float* bn_rm[8];              /* layerN.1.running_mean (updated in place when train_bn != 0) */
    float* bn_rv[8];              /* layerN.1.running_var  (updated in place when train_bn != 0) */
    const float* fc1_w;           /* fc1.weight (1024, 32768), reference flatten order c*256 + h*16 + w */
    const float* fc1_b;           /* fc1.bias (1024) */
    const float* fc2_w;           /* fc2.weight (2, 1024) */
} hrn_shiftnet_params;

size_t hrn_shiftnet_packed_bytes(void);
int hrn_shiftnet_pack(const hrn_shiftnet_params* params, void* packed, size_t packed_bytes, void* stream);
size_t hrn_shiftnet_workspace_bytes(int B);

/* x (B,2,128,128) f32 -> theta (B,2) f32.  `params` supplies the live BatchNorm tensors (affine + running stats) and
 * fc1_w, which is read IN PLACE in the reference's layout (its 134 MB are not part of `packed`); the other conv/fc
 * pointers are not read here (they live in `packed`).
 * train_bn != 0: batch statistics (biased var) and running-stat update with `momentum` (nn.BatchNorm2d train mode);
 * dropout_mask: NULL (eval) or uint8 (B,32768) keep-mask in the reference's flatten order; kept activations x2. */
int hrn_shiftnet_forward(const void* packed, const hrn_shiftnet_params* params, const float* x, int B,
                         int train_bn, float momentum, const unsigned char* dropout_mask, float* theta,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Training path (ShiftNet in .train() mode; `shifts = register_batch(regis_model, ...)` ... `loss.backward()`,
 * src/train.py:176-190).  hrn_shiftnet_forward_train = hrn_shiftnet_forward(train_bn = 1) with every layer's tensors
 * and batch statistics kept in `train_ws`; hrn_shiftnet_backward turns d_theta (B,2) into the parameter gradients,
 * ACCUMULATED (+=) into the buffers of `grads` (conv_w/conv_b/bn_g/bn_b/fc1_w/fc1_b/fc2_w in the parameters' own
 * reference layouts; bn_rm/bn_rv are not read), and, when d_x is not NULL, writes the gradient of the input pairs
 * d_x (B,2,128,128).  `params` are the raw reference-layout tensors, `dropout_mask` the mask the forward used.  Any B > 0:
 * the fc1 kernels take 32 samples per launch and larger batches go through them in slices. */
size_t hrn_shiftnet_train_workspace_bytes(int B);
int hrn_shiftnet_forward_train(const void* packed, const hrn_shiftnet_params* params, const float* x, int B, float momentum,
                               const unsigned char* dropout_mask, float* theta, void* train_ws, size_t train_ws_bytes,
                               void* stream);
int hrn_shiftnet_backward(const hrn_shiftnet_params* params, const float* x, int B, const unsigned char* dropout_mask,
                          const float* d_theta, const hrn_shiftnet_params* grads, float* d_x, void* train_ws,
                          size_t train_ws_bytes, void* stream);
/* The same with a dtype: HRN_DTYPE_F32 (what the three functions above run) or HRN_DTYPE_BF16 - every activation and activation
 * gradient of the workspace ONE bf16 plane (stores round to nearest even), the convolutions, their data and weight gradients one bf16
 * MFMA per product with fp32 accumulation, the conv weights packed to bf16 into the workspace by the forward (from params->conv_w, which
 * must then be set); BatchNorm statistics and every reduction in f32 / f64 as in fp32.  fc1 / fc2 and their backward, x, d_x, theta,
 * d_theta, the running statistics, parameters and parameter gradients: f32 in both modes; `packed` is the fp32 blob of
 * hrn_shiftnet_pack in both.  The workspace (hrn_shiftnet_train_workspace_bytes_dt of the same dtype) is smaller in bf16.  Any other
 * dtype: 0 bytes, and -2 before any launch.  HRN_DTYPE_BF16 also wants `packed` and `train_ws` 256-byte aligned (as any hipMalloc'd
 * block is); otherwise -2 before any launch. */
size_t hrn_shiftnet_train_workspace_bytes_dt(int dtype, int B);
int hrn_shiftnet_forward_train_dt(const void* packed, int dtype, const hrn_shiftnet_params* params, const float* x, int B, float momentum,
                                  const unsigned char* dropout_mask, float* theta, void* train_ws, size_t train_ws_bytes, void* stream);
int hrn_shiftnet_backward_dt(const hrn_shiftnet_params* params, int dtype, const float* x, int B, const unsigned char* dropout_mask,
                             const float* d_theta, const hrn_shiftnet_params* grads, float* d_x, void* train_ws, size_t train_ws_bytes,
                             void* stream);
/* hrn_shiftnet_backward_dt for a partly frozen ShiftNet: a NULL field of `grads` means "not requested" (`grads` itself must not be NULL).
 * A frozen layer's weight / bias gradients and a frozen fc1.weight / fc1.bias / fc2.weight are not computed; the walk back stops at the
 * first layer (from the input) below which nothing is requested, with d_x NULL.  Requested gradients and d_x are bit-identical to the
 * full backward's.  Same arguments, checks, workspace and return codes as hrn_shiftnet_backward_dt.  The other hrn_shiftnet_backward*
 * forms are this function with the dtype fixed or passed on, so they treat a NULL field of `grads` the same way. */
int hrn_shiftnet_backward_sel(const hrn_shiftnet_params* params, int dtype, const float* x, int B, const unsigned char* dropout_mask,
                              const float* d_theta, const hrn_shiftnet_params* grads, float* d_x, void* train_ws, size_t train_ws_bytes,
                              void* stream);

/* ------------------------------------------------------------------ Lanczos */
/* dx (n) f32 -> taps (n,7) f32;  a = 3, N = 7 (the only values the reference's call sites use). */
int hrn_lanczos_kernel(const float* dx, int n, float* taps, void* stream);
/* img (b,c,H,W) f32, shift (c,2) = (dy,dx) per channel -> out (b,c,H,W) f32;  a = 3, N = 7, any p >= 3. */
int hrn_lanczos_shift(const float* img, const float* shift, int b, int c, int H, int W, float* out, void* stream);
/* Backward of hrn_lanczos_shift (autograd through lanczos.lanczos_shift / ShiftNet.transform in apply_shifts,
 * src/train.py:47-63, lanczos.py:47-107): d_img (b,c,H,W) = adjoint of the shift applied to d_out (may be NULL),
 * d_shift (c,2) += gradient through the Lanczos taps, summed over b (may be NULL). */
size_t hrn_lanczos_shift_backward_workspace_bytes(int b, int c, int H, int W);
int hrn_lanczos_shift_backward(const float* img, const float* shift, const float* d_out, int b, int c, int H, int W,
                               float* d_img, float* d_shift, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ loss / score reductions
 * hrn_get_loss     <-  get_loss(srs, hrs, hr_maps, metric)   src/train.py:66-87, with get_crop_mask (:90-106) folded in:
 *                      srs/hrs/hr_maps (B,S,S) f32 -> out (B) f32.  metric: 0 'masked_MSE', 1 'cMSE', 2 'cPSNR' (returns
 *                      -10 log10(cMSE) exactly like the reference); crop: border width forced to mask 0 (0 = none).
 * hrn_shift_cpsnr  <-  shift_cPSNR(np.clip(sr,0,1), hr, hr_map, border_w)   src/Evaluator.py:52-73 (cPSNR :11-43),
 *                      batched: (B,S,S) f32 -> out (B) f32 = max over the (2 border + 1)^2 integer offsets of hr;
 *                      clip != 0 clamps sr to [0,1] first (predict.py:43, train.py:212); workspace: B*(2b+1)^2 doubles.
 *                      Status maps are binary (Evaluator's formula squares the mask; identical for 0/1 maps). */
int hrn_get_loss(const float* srs, const float* hrs, const float* hr_maps, int B, int S, int crop, int metric, float* out, void* stream);
/* The same loss as the differentiable tail of a training step (src/train.py:183-187: loss = -get_loss(srs_shifted, hrs,
 * mask, 'cPSNR')): hrn_get_loss_train also writes stats (B,4) f64 = {n, brightness bias b, cMSE, 0} per sample;
 * hrn_get_loss_backward turns d_out (B) into d_srs (B,S,S) with b held constant, as the reference detaches it (train.py:83):
 * d cMSE / d sr = 2 m (sr + b - hr) / n.  metric: 1 'cMSE' or 2 'cPSNR'.  workspace: fp64 partial sums (fixed-order: reproducible). */
size_t hrn_get_loss_train_workspace_bytes(int B);
int hrn_get_loss_train(const float* srs, const float* hrs, const float* hr_maps, int B, int S, int crop, int metric, float* out,
                       double* stats, void* workspace, size_t workspace_bytes, void* stream);
int hrn_get_loss_backward(const float* srs, const float* hrs, const float* hr_maps, const double* stats, const float* d_out, int B,
                          int S, int crop, int metric, float* d_srs, void* stream);
size_t hrn_shift_cpsnr_workspace_bytes(int B, int border);
int hrn_shift_cpsnr(const float* srs, const float* hrs, const float* hr_maps, int B, int S, int border, int clip, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The shift-searched score as a differentiable training loss: shift_cPSNR's search over the (2 border + 1)^2 integer offsets of hr
 * (src/Evaluator.py:52-73) around get_loss's brightness-corrected cMSE (src/train.py:66-87), on frames of any size and aspect ratio.
 * srs/hrs/hr_maps (B,H,W) f32, H and W > 2 border, border 0..8; with h = H - 2 border, w = W - 2 border, s = srs[border:border+h,
 * border:border+w] (clamped to [0,1] when clip != 0) and, for the offset k = u (2 border + 1) + v, g = hrs[u:u+h, v:v+w], m =
 * hr_maps[u:u+h, v:v+w]:  n_k = sum m, bias_k = sum m (g - s) / n_k, cMSE_k = sum m (s + bias_k - g)^2 / n_k.  k* is the lowest k of
 * minimal cMSE_k among n_k > 0.  metric: 1 'cMSE' -> out = cMSE_k*, 2 'cPSNR' -> out = -10 log10(cMSE_k*) (the reference's sign).
 * hrn_shift_loss_train      <-  shift_cPSNR (Evaluator.py:52-73) over get_loss (train.py:66-87): out (B) f32 and stats (B,4) f64 =
 *                               {n*, bias*, cMSE*, k*}; without a clear pixel at any offset out is NaN and stats {0, 0, NaN, -1}.
 *                               Fixed-order fp64 sums, no atomics: bit-reproducible.
 * hrn_shift_loss_backward   <-  autograd through that loss (Evaluator.py:52-73, train.py:66-87; the bias term's own contribution is
 *                               sum m (s + bias - g) = 0): d_srs (B,H,W), every element written = d_out[b] c m*(s + bias* - g*) at
 *                               the selected offset, c = 2 / n* (cMSE) or -20 / (ln 10 n* cMSE*) (cPSNR); 0 on the border frame,
 *                               where clip clamped s, and for a sample without a clear pixel.  No gradient to hrs / hr_maps.
 * hrn_shift_loss_workspace_bytes: the forward's fp64 partial sums (0 for arguments the entry points refuse). */
size_t hrn_shift_loss_workspace_bytes(int B, int H, int W, int border);
int hrn_shift_loss_train(const float* srs, const float* hrs, const float* hr_maps, int B, int H, int W, int border, int metric, int clip,
                         float* out, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int hrn_shift_loss_backward(const float* srs, const float* hrs, const float* hr_maps, const double* stats, const float* d_out, int B,
                            int H, int W, int border, int metric, int clip, float* d_srs, void* stream);

/* The second score, cSSIM: structural similarity between the clear pixels of the target and the brightness-corrected prediction, searched
 * over the offsets and crops of hrn_shift_loss_train (the project's own definition; tests/cssim_ref.py restates it in fp64).
 * srs/hrs/hr_maps (B,H,W) f32; a map is 0 / non-zero by `!= 0`: a fractional, negative or denormal value is a clear pixel of weight 1 and
 * -0.0 is masked; a +inf in srs is 1 when clip != 0, and when clip == 0 it makes every score of its sample NaN (no k*); border 0..8; h, w, s (clamped to [0,1] when clip != 0, a NaN stays NaN) and, for
 * the offset k = u (2 border + 1) + v, g and m as above; n_k = sum m, bias_k = sum m (g - s) / n_k, or 0 when correct_bias == 0.  The
 * compared pair is X = m g and Y = m (s + bias_k): masked pixels are zero in both.  The window G is separable, sums to 1 and is applied
 * where it fits ("valid": the SSIM map is (h - T + 1) x (w - T + 1), no padding), so H and W must each be >= 2 border + T:
 *   window 0 (gaussian)  T = 11 taps exp(-x^2 / (2 1.5^2)), x = -5..5, normalised in fp64 and rounded to fp32; cov_norm = 1
 *   window 1 (uniform)   T = 7 taps of 1/7; cov_norm = 49/48 (the sample covariance)
 *   mu_x = G X, mu_y = G Y, v_x = cov_norm (G X^2 - mu_x^2), v_y likewise, v_xy = cov_norm (G XY - mu_x mu_y),
 *   C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = data_range > 0,
 *   SSIM = (2 mu_x mu_y + C1) (2 v_xy + C2) / ((mu_x^2 + mu_y^2 + C1) (v_x + v_y + C2)),  score_k = the mean of the map,
 * and score_k = -inf where n_k = 0.  k* is the lowest k of maximal score_k among n_k > 0 under a strict >, so a NaN score is never
 * selected.  out (B) f32 = score_k*, stats (B,4) f64 = {n*, bias*, score*, k*}; without an eligible offset out is NaN and stats {0, 0,
 * NaN, -1}.  scores (B, (2 border + 1)^2) f64, may be NULL: every score_k.  correct_bias = 0, border = 0, window = 1 with the caller's
 * data_range is the reference fork's registration_metrics.compute_ssim(..., use_masks=True) on a common mask (zeroed non-common
 * pixels, skimage's 7 x 7 uniform window and sample covariance, the mean over the un-padded map).  fp32 filters, fp64 sums in a fixed
 * order, no atomics: bit-reproducible, and a sample's result does not depend on the batch around it.  No gradient: it is a score.
 * hrn_shift_cssim_workspace_bytes: the fp64 partial sums (0 for arguments the entry point refuses). */
size_t hrn_shift_cssim_workspace_bytes(int B, int H, int W, int border, int window);
int hrn_shift_cssim(const float* srs, const float* hrs, const float* hr_maps, int B, int H, int W, int border, int window, int clip,
                    int correct_bias, float data_range, float* out, double* stats, double* scores, void* workspace,
                    size_t workspace_bytes, void* stream);
/* cSSIM as a training loss: the gradient of score_k* with respect to srs, with k* HELD FIXED (as hrn_shift_loss_backward holds it) and the
 * bias ATTACHED (unlike the cMSE its term does not cancel: this is the derivative of the number hrn_shift_cssim returns).  The forward of
 * the loss is hrn_shift_cssim itself (scores may be NULL); `stats` is its (B,4) {n*, bias*, score*, k*}.  With s, g, m, n = n*, b = bias*
 * at k*, X = m g, Y = m (s + b), Np = (h - T + 1)(w - T + 1) and, per map pixel, a = mu_x, c = mu_y:
 *   A1 = 2ac + C1,  A2 = 2 v_xy + C2,  B1 = a^2 + c^2 + C1,  B2 = v_x + v_y + C2,
 *   S_c = 2a A2/(B1 B2) - 2c A1 A2/(B1^2 B2),   S_vy = -A1 A2/(B1 B2^2),   S_vxy = 2 A1/(B1 B2),
 *   beta = 2 cov_norm S_vy,   gamma = cov_norm S_vxy,   alpha = S_c - beta c - gamma a,
 *   D_q = [ (G^T alpha)_q + Y_q (G^T beta)_q + X_q (G^T gamma)_q ] / Np     for a crop pixel q,
 *   M   = sum_q m_q D_q / n   (0 when correct_bias == 0),
 *   d score / d srs[border + y, border + x] = pass m (D - M),
 * G^T the adjoint of the "valid" window (the map-sized field, zero outside the map, correlated with the same taps back onto the h x w
 * crop) and pass = 1 where torch.clamp passes a gradient (0 <= s <= 1 before clamping), or everywhere when clip == 0.
 * hrn_cssim_loss_backward  <-  autograd through that score: d_srs (B,H,W), every element written = d_out[b] times the above; exactly 0 on
 *                              the border frame, where clip clamped s, on masked pixels and for a sample without an eligible offset
 *                              (k* = -1).  No gradient to hrs / hr_maps.  fp32 filters, fp64 sums in a fixed order, no atomics:
 *                              bit-reproducible, and a sample's gradient does not depend on the batch around it.
 * hrn_cssim_loss_backward_workspace_bytes: the tiles' fp64 sums (0 for arguments the entry point refuses). */
size_t hrn_cssim_loss_backward_workspace_bytes(int B, int H, int W, int border, int window);
int hrn_cssim_loss_backward(const float* srs, const float* hrs, const float* hr_maps, const double* stats, const float* d_out, int B, int H,
                            int W, int border, int window, int clip, int correct_bias, float data_range, float* d_srs, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The third searched loss, cL1: the brightness-corrected, shift-searched L1 (cMAE) and its smooth form, Charbonnier, over the offsets and
 * crops of hrn_shift_loss_train (the project's own definition; tests/cl1_ref.py restates it in fp64).  srs/hrs/hr_maps (B,H,W) f32, H and
 * W > 2 border, H W < 2^31, border 0..8; h, w, s (clamped to [0,1] when clip != 0) and, for the offset k = u (2 border + 1) + v, g and m
 * as above.  The map is a WEIGHT, as in hrn_shift_loss_train (it is not binarised as cSSIM's is).  With rho(e) = |e| for eps == 0 and
 * sqrt(e^2 + eps^2) otherwise, rho' its derivative (rho'(0) = 0 at eps == 0), eps finite and >= 0:
 *   n_k = sum m,  b_k = sum m (g - s) / n_k,  e = s + b_k - g,  cL1_k = sum m rho(e) / n_k,  sigma_k = sum m rho'(e) / n_k.
 * k* is the lowest k of minimal cL1_k among n_k > 0 under a strict <; a NaN is never selected over a number.  out = cL1_k*, to be
 * minimised as it is (no sign flip, unlike 'cPSNR').
 * hrn_cl1_loss_train      <-  out (B) f32 and stats (B,5) f64 = {n*, b*, cL1*, k*, sigma*}; without a clear pixel at any offset out is NaN
 *                             and stats {0, 0, NaN, -1, 0}.  Two walks over the offsets (|e| does not expand as e^2 does: every b_k must be
 *                             known, over the whole sample, before an absolute value is taken), e and its sign formed in fp64 from the fp64
 *                             bias, fp64 sums in a fixed order, no atomics: bit-reproducible, and a sample's result does not depend on
 *                             the batch around it.
 * hrn_cl1_loss_backward   <-  autograd through that loss with k* held fixed and the bias ATTACHED (unlike the cMSE its term does not
 *                             cancel: this is the derivative of the number returned): d_srs (B,H,W), every element written =
 *                             d_out[b] m* / n* (rho'(e*) - sigma*) at the selected offset; exactly 0 on the border frame, where clip
 *                             clamped s (0 <= s <= 1 passes, as torch.clamp has it; clamped pixels still count in sigma*) and for a
 *                             sample without a clear pixel.  No gradient to hrs / hr_maps.
 * hrn_cl1_loss_workspace_bytes: the tiles' fp64 sums and every offset's {n_k, b_k} (0 for arguments the entry points refuse). */
size_t hrn_cl1_loss_workspace_bytes(int B, int H, int W, int border);
int hrn_cl1_loss_train(const float* srs, const float* hrs, const float* hr_maps, int B, int H, int W, int border, int clip, float eps,
                       float* out, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int hrn_cl1_loss_backward(const float* srs, const float* hrs, const float* hr_maps, const double* stats, const float* d_out, int B, int H,
                          int W, int border, int clip, float eps, float* d_srs, void* stream);

/* ------------------------------------------------------------------ sub-pixel registration of LR views: a masked-NCC grid search
 * The method of the reference fork's registration_search.py / registration_metrics.py (compute_shift_ncc -> recursive_mncc_search ->
 * compute_grid_mncc), on definitions of this project's own; tests/registration_ref.py restates them in fp64 and is what the tests
 * compare against.  ref / ref_mask (B,H,W), views / view_masks (B,V,H,W), all f32; a mask is 0 / non-zero and a NULL mask pointer
 * means all ones.  16 <= H, W <= 128 for the first three entry points (a view resident in one CU's LDS), 16..16384 for the *_scene ones.
 *   shift    s = (dy, dx):  Output(y, x) = Input(y + dy, x + dx) - the order and sign of hrn_lanczos_shift's `shift`, the negative of the
 *            fork's ndi_shift convention.
 *   sampler  S(T, s), per axis: n = floor(d), f = d - n on the fp32 value of d; six taps at sample offsets o = -2..3, k_o = sinc(o - f)
 *            sinc((o - f) / 3), sinc(t) = sin(pi t) / (pi t), k = 0 for |o - f| >= 3, normalised to sum 1; applied along rows, then along
 *            columns.  The footprint of pixel (y, x) is rows y + n_y - 2 .. y + n_y + 3 and columns x + n_x - 2 .. x + n_x + 3; there is
 *            no padding rule: a pixel whose footprint leaves the frame is invalid and its value is 0.  Continuous in s.
 *   mask     V(M, s): the bilinear sample of M at (y + dy, x + dx), zeros outside the frame, (1 - f_y) ((1 - f_x) M00 + f_x M01) + f_y
 *            ((1 - f_x) M10 + f_x M11); a pixel is valid iff the sample is > 0.5 and its footprint is inside the frame.
 *   score    c = M_ref V(M_t, s), n = sum c, t = S(T, s), r = R, both standardised over c: score = sum c (r - mu_r)(t - mu_t) / (n sigma_r
 *            sigma_t), in [-1, 1]; -inf when n = 0 or either variance is <= 0.
 *   grid     centre (cy, cx), width w, P points per axis: d_i = c - w / 2 + i w / (P - 1) in fp64, rounded to fp32; scores[i][j] belongs
 *            to (dy_i, dx_j).  The best point is the first maximum in row-major order (strict >); without a finite score the centre stays
 *            and the level's score is -inf.
 *   search   level k = 0..levels-1 has width w_0 = 2 radius, w_{k+1} = w_k s (fp64), s = 1 / (P - 2), raised to 0.25 if smaller and set
 *            to 0.9 if >= 1; the first centre is (0, 0), every later one the previous level's best point.
 * hrn_mncc_grid    one grid level: centres (B,V,2) f32 = (cy, cx), width in (0, 8] -> scores (B,V,P,P) f32.
 * hrn_mncc_search  the whole search in ONE launch (a workgroup owns a view and walks every level, argmax included): shifts (B,V,2) f32
 *                  = the last best point, trace (B,V,levels,3) f32 = (dy, dx, score) per level, or NULL.  P 3..9, levels 1..16, radius in
 *                  (0, 4].  Its level-k scores are hrn_mncc_grid's, bit for bit.
 * hrn_mncc_apply   out (B,V,H,W) = S(view, shift), out_valid (B,V,H,W) = 1 where V(mask, shift) holds, else 0; shifts (B,V,2).  Invalid
 *                  pixels of `out` are 0.
 * Fixed-order sums, no atomics: bit-reproducible.  -2 before any launch, with hrn_last_error() naming the fault: a null pointer other
 * than a mask or `trace`, B or V not positive, H or W outside 16..128, P, levels, radius or width out of range. */
int hrn_mncc_grid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B, int V,
                  int H, int W, int P, float width, float* scores, void* stream);
int hrn_mncc_search(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W, int P,
                    int levels, float radius, float* shifts, float* trace, void* stream);
int hrn_mncc_apply(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                   float* out_valid, void* stream);
/* The same definitions for frames of any size, 16 <= H, W <= 16384 (the "scene" path, beside hrn_hrnet_forward's tiled inference): a
 * frame is cut into tiles of 64 x 64 pixels, a workgroup stages a tile of the view plus a halo into LDS per level, and a second, small
 * launch per level adds the tiles' fp64 sums in index order, forms the scores and takes the first maximum.  The next level reads its
 * centre from device memory: nothing returns to the host.  Both images are centred on their whole-frame masked means (fixed-order
 * fp64 sums, the mean rounded to fp32) before a score's sums are taken, as above; tiles are never centred apart.
 * hrn_mncc_scene_workspace_bytes  the workspace of the two entry points below; 0 for arguments they refuse.  With T = ceil(H / 64)
 *                  ceil(W / 64) tiles and C = min(64, ceil(H W / 16384)) chunks of a frame's mean:
 *                      16 (B V + B) C  +  48 P^2 B V T  +  8 B V   bytes
 *                  (the chunks' {sum, count}, the tiles' six sums per grid point, the centres): at most the 4 B V H W bytes of `views`
 *                  wherever H, W >= 64.
 * hrn_mncc_grid_scene    as hrn_mncc_grid.  A grid coordinate beyond +-256 is taken as +-256.
 * hrn_mncc_search_scene  as hrn_mncc_search, in 1 + 2 levels launches.  Its level-k scores are hrn_mncc_grid_scene's, bit for bit.
 * hrn_mncc_apply_scene   as hrn_mncc_apply, and bit-identical to it wherever both run.  No workspace.
 * Fixed-order sums, no atomics: bit-reproducible, and a view's result does not depend on the batch around it.  -2 before any launch as
 * above (H or W outside 16..16384; a null workspace; B V T beyond 2^31 - 1), -3 for a workspace that is too small. */
size_t hrn_mncc_scene_workspace_bytes(int B, int V, int H, int W, int P);
int hrn_mncc_grid_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B,
                        int V, int H, int W, int P, float width, float* scores, void* workspace, size_t workspace_bytes, void* stream);
int hrn_mncc_search_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                          int P, int levels, float radius, float* shifts, float* trace, void* workspace, size_t workspace_bytes,
                          void* stream);
int hrn_mncc_apply_scene(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                         float* out_valid, void* stream);
/* The backward of the sampler: out = S(view, shift) is linear in the view and C^1 in the shift - the six normalised taps are continuous
 * with their first derivative across whole-pixel boundaries, because L3'(+-3) = 0 with L3(t) = sinc(t) sinc(t / 3).  valid / d_out
 * (B,V,H,W) are hrn_mncc_apply_scene's out_valid and the gradient that arrives at `out`.  With (n_y, f_y), (n_x, f_x) and the taps k of
 * the view's shift as above:
 *   g         = d_out where `valid` is non-zero AND the pixel's 6 x 6 footprint lies inside the frame, else 0.  The footprint is tested
 *               again here, so whatever `valid` holds nothing outside a frame is read.
 *   d_views   (B,V,H,W): d_views(p, q) = sum_{a, b = -2..3} k^y_a k^x_b g(p - n_y - a, q - n_x - b), g zero outside the frame: the adjoint
 *               as a gather (one shift per view) - the sampler's two passes with the taps reversed, the whole parts (-n_y - 1, -n_x - 1)
 *               and zero padding.  Every element is written; exactly 0 where no valid pixel's footprint reaches.
 *   d_shifts  (B,V,2): d_shifts[., 0] = sum_pixels g dS/ddy, where dS/ddy takes the taps k'^y along columns and k^x along rows; [., 1] is
 *               the mirror.  k'_o = (u'_o - k_o sum u') / sum u with u_o = L3(o - f), u'_o = -L3'(o - f), formed in fp64 per view and
 *               rounded to fp32 as k is.  A pixel's product is fp32; every sum is fp64 in a fixed order (thread, wave, waves, tiles in
 *               index order), rounded to fp32 once.  Exactly 0 for a view without a valid pixel, and for a coordinate at or beyond +-256
 *               (or a NaN): the sampler clamps it there, and the clamp has zero slope.
 * There is no gradient to the masks or to `valid`: they are piecewise constant in the shift.
 * hrn_mncc_apply_backward_workspace_bytes  16 B V T bytes, T = ceil(H / 64) ceil(W / 64): the tiles' two fp64 sums; 0 for arguments the
 *                  entry point refuses.
 * hrn_mncc_apply_backward  either of d_views / d_shifts may be NULL: that half is not run (one launch for d_views, two for d_shifts);
 *                  both NULL is refused.  `views` and `workspace` are needed only for d_shifts and may be NULL without it.  16 <= H, W
 *                  <= 16384.  No atomics: both results are bit-reproducible, and a view's does not depend on the batch around it.  -2
 *                  before any launch as above, -3 for a workspace that is too small. */
size_t hrn_mncc_apply_backward_workspace_bytes(int B, int V, int H, int W);
int hrn_mncc_apply_backward(const float* views, const float* shifts, const float* valid, const float* d_out, int B, int V, int H, int W,
                            float* d_views, float* d_shifts, void* workspace, size_t workspace_bytes, void* stream);
/* The sub-pixel searched loss: the brightness-corrected cMSE / cPSNR of the prediction REGISTERED to its target by
 * the search above, scored by the cMSE itself instead of the NCC (which is invariant to gain and so is not the score);
 * tests/subpixel_ref.py restates it in fp64.  srs / hrs / hr_maps (B,H,W) f32, 16 <= H, W <= 16384, border 0..8 and below half of each
 * side.  A shift s = (dy, dx) means S(sr, s)(p) = sr(p + s), S the six-tap sampler above.  For one sample:
 *   m0        hr_map != 0 (the map is binary here, as in cSSIM) and p at least `border` from every frame edge.
 *   c(s)      m0 and the 6 x 6 footprint of p at s inside the frame; the prediction has no mask of its own.  n(s) = |c|.
 *   b(s)      the mean over c of hr - S(sr, s).
 *   cMSE(s)   the mean over c of (S(sr, s) + b - hr)^2, clamped at 0.  It is formed in fp64 from the level's six sums n, sum t, sum r,
 *             sum t^2, sum r^2, sum r t over c, t = S(sr - mean sr, s) and r = hr - mean hr (whole-frame means, of hr under m0, rounded to
 *             fp32 as above), as (sum t^2 + sum r^2 - 2 sum r t - (sum t - sum r)^2 / n) / n: a constant taken off either image cancels.
 *   search    `levels` grids of P x P points as above (grid, search: the first centre (0, 0), w_0 = 2 radius, the ratio rule, fp32
 *             coordinates), the best point the first maximum of -cMSE in row-major order (strict >, compared in fp64), -inf where n = 0;
 *             a NaN is never taken; without a point the centre stays.
 *   result    cMSE (metric 1) or cPSNR = -10 log10 cMSE (metric 2, the reference's sign: negate to minimise) at the last level's point
 *             s*.  A sample whose last level has no counted pixel at any point - as one without a clear pixel inside the border frame -
 *             gives NaN.
 * hrn_subpixel_loss_train     <-  out (B) f32, stats (B,8) f64 = {n*, b* in image units, cMSE*, dy*, dx*, mean sr, mean hr under m0, the
 *                                 centred bias (sum r - sum t) / n*} ({0, 0, NaN, cy, cx, means, 0} for a NaN sample), trace (B,levels,3)
 *                                 f32 = (dy, dx, cMSE) of every level's point, or NULL.  2 + 2 levels launches; nothing returns to the
 *                                 host, no atomics, fixed-order fp64 sums: bit-reproducible, and a sample's result does not depend on the
 *                                 batch around it.
 * hrn_subpixel_loss_backward  <-  autograd through that loss with s* held fixed; the bias term cancels for a square, so with e = S(sr, s*)
 *                                 + b* - hr (formed as t + centred bias - r in fp64, t and r by the forward's operations on the means of
 *                                 `stats`): g = d_out[b] factor 2 c e / n*, factor 1 for cMSE and -10 / (ln 10 cMSE*) for cPSNR, and d_srs
 *                                 (B,H,W) = the sampler's adjoint of g (d_views above).  Every element is written; exactly 0 where no
 *                                 counted pixel's footprint reaches, and everywhere for a NaN sample.  No gradient to hrs / hr_maps or to
 *                                 the shift.  Two launches.
 * hrn_subpixel_loss_workspace_bytes  one size for both entry points, 0 for arguments they refuse: the larger of the forward's (m0 and
 *                                 hrn_mncc_scene_workspace_bytes(B, 1, H, W, P)) and the backward's (g, c and the fp32 shifts: 8 B H W +
 *                                 8 B, each plane rounded up to 16 bytes).  The backward takes any P's size.
 * -2 before any launch, with hrn_last_error() naming the fault: a null pointer other than `trace`, B not positive, a side outside
 * 16..16384, border outside 0..8 or not below half of each side, P outside 3..9, levels outside 1..16, radius outside (0, 4], a metric
 * other than 1 or 2, B T beyond 2^31 - 1 workgroups; -3 for a workspace that is too small.  `clip` is not offered. */
size_t hrn_subpixel_loss_workspace_bytes(int B, int H, int W, int P);
int hrn_subpixel_loss_train(const float* srs, const float* hrs, const float* hr_maps, int B, int H, int W, int border, int P, int levels,
                            float radius, int metric, float* out, double* stats, float* trace, void* workspace, size_t workspace_bytes,
                            void* stream);
int hrn_subpixel_loss_backward(const float* srs, const float* hrs, const float* hr_maps, const double* stats, const float* d_out, int B,
                               int H, int W, int border, int metric, float* d_srs, void* workspace, size_t workspace_bytes, void* stream);
/* A shift per block of every view - a shift field - on the scene path's tiles.  `block` is a multiple of 64 in
 * 64..4096.  An axis of length L has n = max(1, (L + block / 2) / block) blocks; block i covers [i block, (i + 1) block) and the last one
 * runs to L, so a remainder below half a block joins its neighbour and every block is a union of whole 64-pixel tiles.
 *   local score   of block (i, j) at a shift: the score above with the reference mask set to zero outside the block.  Both images stay
 *                 centred on their whole-frame means, and a block's sums are its tiles' sums added in tile-index order.
 *   local search  per (view, block): `levels` levels of the grid rule above, the first centre init[b, v] ((0, 0) for a NULL `init`).  A
 *                 level without a finite score keeps its centre.  With n the count of common valid pixels at the last level's best
 *                 point, the block is ok when that point's score is finite and n >= min_valid * (the block's area in pixels), compared
 *                 in fp64; field[b, v, i, j] is the best point of an ok block and init[b, v] otherwise.
 *   field at (y, x)  nodes at the centres ((r0 + r1 - 1) / 2, (c0 + c1 - 1) / 2) of the blocks' rectangles.  Per axis k = the last node at
 *                 or before the pixel, within [0, n - 2], t = clamp((p - node_k) / (node_{k+1} - node_k), 0, 1) (constant beyond the outer
 *                 nodes; t = 0 with one block), and per component, in fp64 and in this order, (1 - ty) ((1 - tx) N00 + tx N01) + ty ((1 -
 *                 tx) N10 + tx N11), rounded to fp32.
 * hrn_mncc_local_blocks  n for an axis of length L; 0 for a `block` that is refused or L outside 1..16384.
 * hrn_mncc_local_workspace_bytes  0 for arguments hrn_mncc_search_local refuses; else, with T and C as above and by x bx blocks,
 *                      16 (B V + B) C  +  48 P^2 B V T  +  8 B V by bx   bytes.
 * hrn_mncc_search_local  init (B,V,2) or NULL; field (B,V,by,bx,2) f32; trace (B,V,by,bx,levels,3) = (dy, dx, score) per level, or NULL;
 *                 ok (B,V,by,bx) f32 1 / 0, or NULL; min_valid in [0, 1].  1 + 2 levels launches, nothing returns to the host.  With one
 *                 block, NULL init and min_valid 0, field and trace are hrn_mncc_search_scene's shifts and trace bit for bit.
 * hrn_mncc_apply_field  out (B,V,H,W) = S(view, the field at the pixel) and out_valid = V(mask, the same), each pixel by its own shift;
 *                 invalid pixels of `out` are 0.  A constant field gives hrn_mncc_apply_scene's bits.  No workspace.
 * Fixed-order sums, no atomics: bit-reproducible.  -2 before any launch as above (also: a block that is no multiple of 64 in 64..4096; B V
 * by bx or B V T beyond 2^31 - 1; min_valid outside [0, 1]), -3 for a workspace that is too small. */
int hrn_mncc_local_blocks(int L, int block);
size_t hrn_mncc_local_workspace_bytes(int B, int V, int H, int W, int P, int block);
int hrn_mncc_search_local(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init, int B, int V,
                          int H, int W, int P, int levels, float radius, int block, float min_valid, float* field, float* trace, float* ok,
                          void* workspace, size_t workspace_bytes, void* stream);
int hrn_mncc_apply_field(const float* views, const float* view_masks, const float* field, int B, int V, int H, int W, int block, float* out,
                         float* out_valid, void* stream);

/* ------------------------------------------------------------------ coarse-to-fine: a masked pyramid under the scene search
 * Nothing in the reference stands behind these: its search starts at (0, 0) with a fixed reach.  hrn_mncc_search_scene reaches `radius`
 * <= 4 pixels from (0, 0); beyond that it returns a confident wrong shift.  A pyramid of K octaves reaches radius 2^K pixels.
 * tests/registration_pyramid_ref.py restates all of this in fp64.
 *   reduce2       a plane (H, W) with a mask -> a plane (H / 2, W / 2) with a mask (integer halves; sides 32..16384, odd sides allowed).
 *                 Weights w = [1, 3, 3, 1] / 8 per axis; coarse pixel (Y, X) reads fine rows 2Y - 1 .. 2Y + 2 and fine columns 2X - 1 ..
 *                 2X + 2.  m = 1 where the fine pixel is inside the frame and clear (mask != 0; a NULL mask: every pixel of the frame is
 *                 clear), else 0.  den = sum over the 16 taps of w_a w_b m, num = sum of w_a w_b (m ? x : 0), taps in row-major order,
 *                 num by fused multiply-adds in fp32.  The coarse pixel is clear iff den > 0.5 (V(M, s)'s threshold); its value is num /
 *                 den when clear and exactly 0 otherwise; the coarse mask is always written, f32 1 / 0.  den adds multiples of 1/64 up to
 *                 1, so it is exact in fp32 and the coarse mask equals its fp64 restatement everywhere.  The filter is even and
 *                 symmetric and reference and view are reduced alike: a fine shift d is a coarse shift d / 2, with no offset.
 *   search from a centre   hrn_mncc_search_scene with the first level's centre read from init (B,V,2) instead of (0, 0); nothing else
 *                 differs.  A NULL init is hrn_mncc_search_scene, bit for bit.
 *   pyramid search  K = octaves in 0..6.  Octaves 1..K of the views with their masks and of the reference with its mask are built by
 *                 reduce2, octave k from octave k - 1.  Octave K is searched from (0, 0) with `radius`; each octave k < K from 2 x (the
 *                 shift of octave k + 1) - exact in fp32 - with `refine_radius`.  Octave 0 takes `levels` levels, every other octave
 *                 `coarse_levels`.  A view without a finite score at an octave keeps its centre, as in the search.  With K = 0 the result
 *                 is hrn_mncc_search_scene's bit for bit.  The reach is radius 2^K pixels of the frame.
 * hrn_mncc_reduce2  x (N,H,W), mask (N,H,W) or NULL -> out (N,H/2,W/2), out_mask (N,H/2,W/2).  One launch, no workspace.
 * hrn_mncc_search_scene_from  hrn_mncc_search_scene's arguments and workspace (hrn_mncc_scene_workspace_bytes) plus init (B,V,2) or NULL.
 * hrn_mncc_pyramid_workspace_bytes  0 for arguments hrn_mncc_search_pyramid refuses (radii and levels aside); else, with H_k = H >> k, W_k
 *                 = W >> k and r16 rounding up to a multiple of 16,
 *                     sum_{k=1..K} r16(8 (B V + B) H_k W_k)  +  r16(hrn_mncc_scene_workspace_bytes(B, V, H, W, P))  +  16 B V   bytes:
 *                 the reduced views, view masks, references and reference masks of every octave, the scene search's workspace of the base
 *                 size (a coarser octave uses its front), and two (B,V,2) centre buffers.  The workspace must be 16-byte aligned.
 * hrn_mncc_search_pyramid  shifts (B,V,2) in pixels of the frame; trace (B,V,K+1,3) = (dy, dx, score) or NULL: row j is the last level of
 *                 octave K - j, in that octave's pixels - coarsest first, row K is `shifts` and its score.  2 K + (1 + 2 levels) + K (1 + 2
 *                 coarse_levels) launches; nothing returns to the host at any point.
 * Fixed-order arithmetic, no atomics: bit-reproducible.  -2 before any launch, with hrn_last_error() naming the fault: what
 * hrn_mncc_search_scene refuses; reduce2: N not positive, a side outside 32..16384, N ceil(H/32) ceil(W/128) beyond 2^31 - 1; the
 * pyramid: octaves outside 0..6, coarse_levels outside 1..16, refine_radius outside (0, 4], radius 2^octaves > 128, min(H, W) >> octaves
 * < 16.  -3 for a workspace that is too small. */
int hrn_mncc_reduce2(const float* x, const float* mask, int N, int H, int W, float* out, float* out_mask, void* stream);
int hrn_mncc_search_scene_from(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init, int B,
                               int V, int H, int W, int P, int levels, float radius, float* shifts, float* trace, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t hrn_mncc_pyramid_workspace_bytes(int B, int V, int H, int W, int P, int octaves);
int hrn_mncc_search_pyramid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                            int P, int octaves, int levels, float radius, int coarse_levels, float refine_radius, float* shifts, float* trace,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ optimiser
 * hrn_adam_step  <-  optimizer.step() of torch.optim.Adam (src/train.py:191, :252), one launch over a flat fp32 buffer
 *                    holding every parameter of both models (the buffer the gradient all-reduce also works on):
 *                    g += weight_decay p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *                    p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).  step counts from 1. */
int hrn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, void* stream);

/* The guarded step (csrc/optim_guard.hip): clipping by the global gradient norm, a skip when any gradient element is not finite,
 * decoupled weight decay (AdamW) and an exponential moving average of the weights, with nothing returning to the host.  Per step:
 * hrn_grad_sumsq once per parameter group, then hrn_optim_prepare and hrn_adam_step_ex once per group, all on one stream.
 *
 * hrn_optim_ctl  the step-control block of one group, 48 bytes of device memory, zero before the first step.  The layout (offsets
 *                in bytes) is part of the ABI: the caller reads norm and the counters from it and may preset the counters.
 *                    0 int64 applied         steps applied so far (the `step` of the bias corrections)
 *                    8 int64 skipped         steps skipped because a gradient element was not finite
 *                   16 double norm           sqrt of the sum of squares of the finite gradient elements of every group, before clipping
 *                   24 float coef            min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient, taken in fp64
 *                                            and rounded once; exactly 1 with max_norm <= 0 (no clipping)
 *                   28 float step_size       lr / (1 - beta1^applied)
 *                   32 float inv_bc2_sqrt    1 / sqrt(1 - beta2^applied), both in fp64 as hrn_adam_step takes them on the host
 *                   36 float lr
 *                   40 int skip              1: hrn_adam_step_ex writes nothing
 *                   44 int reserved
 * hrn_grad_sumsq_workspace_bytes  16 bytes per block of the first launch; the grid is a function of n alone.
 * hrn_grad_sumsq out[0] = sum of g^2 over the finite elements, each square exact in fp64 and the additions in a fixed order (no atomics:
 *                bit-reproducible, whatever else runs); out[1] = the number of non-finite elements (+-inf, NaN), as a double.  Two launches.
 *                n == 0 launches only the second and writes {0, 0}.  fp32 sums would overflow at |g| ~ 2e19; these do not.
 * hrn_optim_prepare  sums (n_groups, 2): every group's hrn_grad_sumsq output.  Writes ctl[group] (ctl: the array of n_groups blocks) for the
 *                group whose lr / betas are given: total = the groups' finite sums added in index order, norm = sqrt(total) (always written);
 *                skip = any group has a non-finite element.  Skipping: skipped += 1, skip = 1, and every other field stays as the last
 *                applied step left it - a skipped step does not advance the bias corrections, as a skipped optimizer.step() does not
 *                count.  Otherwise applied += 1, skip = 0 and coef, step_size, inv_bc2_sqrt, lr as above.  One wave.
 * hrn_adam_step_ex  ctl: the block of this group.  skip set: returns without writing (params, moments and ema keep their bits).  Else
 *                    g' = coef g (+ weight_decay p unless decoupled);  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
 *                    p = p (1 - lr weight_decay) [decoupled only] - step_size m / (sqrt(v) inv_bc2_sqrt + eps);
 *                    ema = ema_decay ema + (1 - ema_decay) p  [ema_or_null given; p is the new value; taken in fp64, rounded once].
 *                grads is never written: the clipped gradient exists in registers only (clip_grad_norm_ rescales .grad in place).
 *                16 B read + 12 B written per parameter, + 4 + 4 with the EMA.
 * -2 before any launch, hrn_last_error() naming the argument: a null pointer, a buffer that is not 16-byte aligned, n_groups outside
 * 1..HRN_OPTIM_MAX_GROUPS, group outside 0..n_groups-1, a beta outside [0, 1), ema_decay outside [0, 1) when ema_or_null is given, a
 * workspace smaller than hrn_grad_sumsq_workspace_bytes(n). */
#define HRN_OPTIM_MAX_GROUPS 8
typedef struct hrn_optim_ctl {
    int64_t applied, skipped;
    double norm;
    float coef, step_size, inv_bc2_sqrt, lr;
    int skip, reserved;
} hrn_optim_ctl;
size_t hrn_grad_sumsq_workspace_bytes(size_t n);
int hrn_grad_sumsq(const float* grads, size_t n, double* out, void* ws, size_t ws_bytes, void* stream);
int hrn_optim_prepare(const double* sums, int n_groups, int group, float max_norm, float lr, float beta1, float beta2,
                      hrn_optim_ctl* ctl, void* stream);
int hrn_adam_step_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_or_null, size_t n,
                     float beta1, float beta2, float eps, float weight_decay, int decoupled, float ema_decay,
                     const hrn_optim_ctl* ctl, void* stream);

/* ------------------------------------------------------------------ input pipeline: batch assembly on the device
 * hrn_collate_device  <-  ImagesetDataset.load_batch (highres-net_amd/DataLoader.py) from imagesets decoded once into HBM:
 *   lr_arena / hr_arena : uint16 samples of every stored LR view / HR image, each image starting at a multiple of 4 elements;
 *                         lr_elems / hr_elems their sizes (multiples of 4).  hr_arena may be NULL when hrs is NULL.
 *   sm_arena            : uint8 status maps (any non-zero sample -> 1.0), same layout rules, sm_elems its size
 *   plan                : (B, HRN_COLLATE_META + min_L) int64, one row per sample:
 *                         hr_off, sm_off, side (stored LR side; HR / SM are 3 * side), row, col (patch corner in LR pixels:
 *                         row first, as get_patch), then min_L LR offsets in use order, -1 for a padding slot.
 *                         hr_off -1: that sample's HR plane is zeros.  Offsets are in elements of the arena.
 *   S                   : output LR side (the patch size, or side for whole images)
 *   lrs (B,min_L,S,S), alphas (B,min_L), hrs (B,3S,3S) or NULL, maps (B,3S,3S): f32 outputs, all written by ONE launch,
 *   padding included: lrs / hrs = (float)((double)u / 65535.0), alphas = 1 for a used slot and 0 for a padding slot.
 * A plan row whose image lies outside its arena or is not 4-aligned, whose corner leaves the stored image, or whose side is
 * not in 1..2^20 gives NaN planes (never an out-of-bounds read); the alpha of such an LR slot stays 1.  Enqueues on `stream`;
 * no synchronisation. */
int hrn_collate_device(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                       const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S,
                       float* lrs, float* alphas, float* hrs, float* maps, void* stream);
/* The same at target scale 2, 3 or 4 (anything else: -2 before any launch): the stored HR / SM images are scale * side,
 * hrs / maps are (B, scale*S, scale*S) and the HR / SM window starts at (scale*row, scale*col).  The plan row layout does
 * not change.  hrn_collate_device is this call with scale = 3. */
int hrn_collate_device_s(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                         const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale,
                         float* lrs, float* alphas, float* hrs, float* maps, void* stream);
/* The same with flip / rotate augmentation (nothing in the reference stands behind this one: its loader never augments;
 * highres-net_amd/hrnet_hip/augment.py states the rule and is what the tests compare against).  codes: device array of B
 * int32, one per sample, or NULL for identity (hrn_collate_device_s is this call with NULL).  A code t in 0..7 acts on every
 * cropped window of the sample - each LR slot (n = S), the SM and the HR window (n = scale*S) - after the crop:
 *     i' = t & 2 ? n-1-i : i,  j' = t & 1 ? n-1-j : j,  out[i][j] = window[t & 4 ? (j', i') : (i', j')]
 * (transpose, then flip rows, then flip columns).  Padding slots stay zeros with alpha 0 and a sample without HR keeps its
 * zero HR plane.  The codes live on the device, so a code outside 0..7 cannot be refused here: every plane of that sample
 * is NaN (alphas as usual), other samples are unaffected, and nothing is read out of bounds.  Still one launch. */
int hrn_collate_device_a(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                         const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale,
                         float* lrs, float* alphas, float* hrs, float* maps, const int32_t* codes, void* stream);
/* The same with the LR quality masks (the QM*.png of the PROBA-V imagesets; the reference never reads them into a batch, they
 * are the `lr_masks` of hrn_mncc_*).  qm_arena: uint8, one byte per LR sample, 1 clear / 0 not (any non-zero byte counts as
 * clear), laid out with exactly the LR arena's element offsets - the mask of the view at LR offset o is at QM offset o - so
 * qm_elems must equal lr_elems and the plan row does not change; 4-byte aligned.  lr_masks: out (B, min_L, S, S) f32, 1.0 / 0.0:
 * slot v of sample b is the window of lrs[b][v] cut from that view's mask and put through the sample's code; a padding slot is
 * zeros, a bad plan row or a bad code makes it NaN like the LR plane beside it.  qm_arena and lr_masks are both NULL (then this is
 * hrn_collate_device_a, qm_elems ignored) or both given; anything else, or qm_elems != lr_elems: -2 before any launch.  Still
 * one launch for all five outputs. */
int hrn_collate_device_m(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                         const uint8_t* sm_arena, int64_t sm_elems, const uint8_t* qm_arena, int64_t qm_elems, const int64_t* plan,
                         int B, int min_L, int S, int scale, float* lrs, float* alphas, float* hrs, float* maps, float* lr_masks,
                         const int32_t* codes, void* stream);

/* ------------------------------------------------------------------ flip / rotate self-ensemble at inference
 * Nothing in the reference stands behind these two: its predict.py runs one orientation.  highres-net_amd/hrnet_hip/augment.py states
 * the rule (apply, inverse, expand, mean_inverse) and is what the tests compare against, bit for bit.  A code t in 0..7 acts on an
 * (H, W) plane as in hrn_collate_device_a: transpose if t & 4, then flip rows if t & 2, then flip columns if t & 1.
 *   codes : the member list, a HOST array of K int32 (1 <= K <= 8), each in 0..7, all distinct.  It is read and validated during
 *           the call, before any launch, and reaches the kernel by value; the caller may free it as soon as the call returns.
 *   hrn_dihedral_expand : x (N,H,W) f32 -> out (K,N,H,W) f32, member-major: out[k][n] = apply(x[n], codes[k]).  One launch.
 *   hrn_dihedral_mean   : y (K,N,H,W) f32 -> out (N,H,W) f32.  With m_k = apply(y[k][n], inverse(codes[k])):
 *                             out[n] = r * ((..((m_0 + m_1) + m_2)..) + m_{K-1}),   r = (float)(1.0 / K)
 *                         i.e. fp32 adds in member order and ONE fp32 multiply.  One launch, no atomics, deterministic.
 * x / y and out are device pointers and must not overlap.  Non-square planes are accepted when no code transposes.
 * -2 before any launch, with hrn_last_error() naming the fault: a null pointer, K outside 1..8, a code outside 0..7, a duplicate
 * code, a code with `t & 4` (the transpose bit) set while H != W, N / H / W not positive, a side above 32768, or (16-byte path) 2^24
 * or more 32 x 32 tiles in all. */
int hrn_dihedral_expand(const float* x, int N, int H, int W, const int32_t* codes, int K, float* out, void* stream);
int hrn_dihedral_mean(const float* y, int N, int H, int W, const int32_t* codes, int K, float* out, void* stream);

/* ------------------------------------------------------------------ tiled inference: scenes of any size and aspect ratio
 * No counterpart in the reference, which predicts a square chip whole.  highres-net_amd/hrnet_hip/tiling.py states the rule (halo,
 * axis_plan, plan, gather, scatter) and is what the tests compare against, bit for bit.
 *
 * hrn_hrnet_halo (no counterpart in the reference): R = 2 + 2 * num_layers + 3 * floor(log2 V), the distance in LR pixels beyond
 * which an LR pixel cannot influence an SR pixel (stem conv, two convs per encoder block, the encoder's final conv, three convs per
 * fusion level; everything else acts per pixel).  -2 for num_layers outside 0..HRN_MAX_RES_LAYERS or V < 1.
 *
 * The plan of an (H, W) scene for square windows of side t <= min(H, W) and halo R: along an axis of length L, with k = t - 2R,
 *     window i :  core_lo = i == 0 ? 0 : (t - R) + (i - 1) * k,   start = min(max(core_lo - R, 0), L - t),
 *                 core_hi = start + t == L ? L : start + t - R;      1 window if L == t, else ceil((L - 2R) / k)
 * and the scene's windows are the row-major product (rows of windows first) of the plans of H and W.  Every window lies inside
 * the scene, the cores [core_lo, core_hi) partition it, and every core edge is on the scene's border or at least R from its
 * window's edge - so a window's forward predicts its core exactly as the whole frame's forward does.
 *
 * hrn_tile_count (no counterpart in the reference): the number of windows of that plan (>= 1), so that a C caller can size its
 * loop; -2 for a plan the two kernels refuse.  Host only.
 *
 * hrn_tile_gather (no counterpart in the reference): lrs (B,V,H,W) f32 -> out (w1-w0, B, V, t, t) f32, window-major, the windows
 * w0 <= w < w1 of the plan.  One launch.
 * hrn_tile_scatter (no counterpart in the reference): srs (w1-w0, B, 1, S t, S t) f32, the forwards of those windows -> their cores
 * in out (B, 1, S H, S W) f32, S = scale in {2, 3, 4}.  Every output pixel of a core is written once; nothing outside the cores
 * of [w0, w1) is touched, so scattering every window of the plan, in any chunks and any order, fills `out` exactly.  One launch.
 * The geometry is computed on the device from (H, W, t, R, window index): no table, no upload, graph-capturable.  Rows whose
 * source and destination are equally aligned move by 16-byte loads and stores, the others per element; any 4-byte aligned pointer
 * is accepted.  The two buffers of a call must not overlap.
 * -2 before any launch, with hrn_last_error() naming the fault: a null pointer, a size that is not positive, t > min(H, W),
 * t < 2R + 1 while the scene needs more than one window, [w0, w1) empty or outside the plan, a scale outside 2..4, H * W (gather)
 * or S H * S W (scatter) beyond 32-bit in-plane offsets, or 2^31 or more window rows in one call. */
int hrn_hrnet_halo(int num_layers, int V);
int hrn_tile_count(int H, int W, int t, int R);
int hrn_tile_gather(const float* lrs, int B, int V, int H, int W, int t, int R, int w0, int w1, float* out, void* stream);
int hrn_tile_scatter(const float* srs, int B, int H, int W, int t, int R, int scale, int w0, int w1, float* out, void* stream);

/* hrn_resample_targets: HR images (elem_bytes 2, uint16) or status maps (elem_bytes 1, uint8, 0 / non-zero) stored at
 * n_in x n_in resampled to n_out x n_out, for a cache whose target scale differs from the ratio the files were stored at
 * (DataLoader.DeviceImagesetCache, resample_targets=True).  One launch for all `n_jobs` images (1..65535):
 *   jobs                  : (n_jobs, 2) int64: element offset of the source image in `src`, of the result in `dst`
 *   first, count, weights : the separable filter, one row per output sample j (used for rows and for columns):
 *                           source taps first[j] .. first[j] + count[j] - 1 with weights[j * HRN_RESAMPLE_TAPS + t], fp64,
 *                           computed on the host (hrnet_hip/resample.py: Lanczos-3, widened when shrinking, rows normalised)
 *   uint16 : v = sum_r w_r (sum_c w_c u[r][c]) in fp64, clipped to [0, 65535], rounded half-to-even
 *   uint8  : 1 if every source sample under a non-zero weight (both axes) is non-zero, else 0
 * n_in : n_out must be R : S for some R, S in {2, 3, 4}.  A job that does not fit `src_elems` / `dst_elems` writes nothing;
 * table entries are clamped to the source image (never an out-of-bounds read).  Deterministic, no atomics. */
#define HRN_RESAMPLE_TAPS 12
int hrn_resample_targets(const void* src, int64_t src_elems, void* dst, int64_t dst_elems, int elem_bytes,
                         const int64_t* jobs, int n_jobs, int n_in, int n_out, const int32_t* first, const int32_t* count,
                         const double* weights, void* stream);

/* ------------------------------------------------------------------ built-in kernel timing (hipEvent pairs)
 * The reference has no profiling hooks; these exist so that bench.py can state, live, the
 * achieved TFLOP/s / GB/s of each kernel family against the gfx950 roofline.  enable(1) clears the table and starts
 * recording on every subsequent launch; enable(0) stops.  get() synchronises the recorded events (host blocks). */
int hrn_profile_enable(int on);
int hrn_profile_count(void);
int hrn_profile_get(int idx, char* name, int name_len, long* launches, double* total_ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* HRNET_HIP_H */
