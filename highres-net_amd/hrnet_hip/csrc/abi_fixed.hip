// The entry points of include/hrnet_hip.h that are another entry point with an argument fixed: scale = 3, dtype = HRN_DTYPE_F32, no
// input gradients, no augmentation codes.  Each is one `return` of the general form, which does the checking and the work (api.hip, train.hip,
// shiftnet_bwd.hip, collate.hip).  Host code only: this file has no kernel.
#include "../../../include/hrnet_hip.h"

extern "C" {

// ---- HRNet, inference: scale = 3
size_t hrn_hrnet_packed_bytes(int dtype, int num_layers) { return hrn_hrnet_packed_bytes_s(dtype, num_layers, 3); }

int hrn_hrnet_pack(const hrn_hrnet_params* P, int dt, void* packed, size_t packed_bytes, void* stream) {
    return hrn_hrnet_pack_s(P, dt, 3, packed, packed_bytes, stream);
}

int hrn_hrnet_forward(const void* packed, int dt, int nl, int alpha_residual, const float* lrs, const float* alphas, int B, int V, int H, int W,
                      float* sr, void* ws, size_t ws_bytes, void* stream) {
    return hrn_hrnet_forward_s(packed, dt, nl, 3, alpha_residual, lrs, alphas, B, V, H, W, sr, ws, ws_bytes, stream);
}

int hrn_decoder_forward(const void* packed, int dt, int nl, const void* fused, int N, int H, int W, float* sr, void* stream) {
    return hrn_decoder_forward_s(packed, dt, nl, 3, fused, N, H, W, sr, stream);
}

// ---- HRNet, training: fp32 at scale 3; a dtype at scale 3; no input gradients (d_lrs = d_alphas = NULL)
int hrn_hrnet_forward_train(const void* pk, int nl, int alpha_residual, const float* lrs, const float* alphas, int B, int V, int H, int W,
                            float* sr, void* tws, size_t tws_bytes, void* stream) {
    return hrn_hrnet_forward_train_s(pk, HRN_DTYPE_F32, nl, 3, alpha_residual, lrs, alphas, B, V, H, W, sr, tws, tws_bytes, stream);
}

int hrn_hrnet_forward_train_dt(const void* pk, int dt, int nl, int alpha_residual, const float* lrs, const float* alphas, int B, int V, int H,
                               int W, float* sr, void* tws, size_t tws_bytes, void* stream) {
    return hrn_hrnet_forward_train_s(pk, dt, nl, 3, alpha_residual, lrs, alphas, B, V, H, W, sr, tws, tws_bytes, stream);
}

int hrn_hrnet_backward(const void* pk, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas, int B, int V,
                       int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, void* tws, size_t tws_bytes, void* stream) {
    return hrn_hrnet_backward_sel(pk, HRN_DTYPE_F32, 3, Pr, alpha_residual, lrs, alphas, B, V, H, W, d_sr, Gr, nullptr, nullptr, tws, tws_bytes,
                                  stream);
}

int hrn_hrnet_backward_dt(const void* pk, int dt, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas, int B,
                          int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, void* tws, size_t tws_bytes, void* stream) {
    return hrn_hrnet_backward_sel(pk, dt, 3, Pr, alpha_residual, lrs, alphas, B, V, H, W, d_sr, Gr, nullptr, nullptr, tws, tws_bytes, stream);
}

int hrn_hrnet_backward_s(const void* pk, int dt, int scale, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas,
                         int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, void* tws, size_t tws_bytes, void* stream) {
    return hrn_hrnet_backward_sel(pk, dt, scale, Pr, alpha_residual, lrs, alphas, B, V, H, W, d_sr, Gr, nullptr, nullptr, tws, tws_bytes, stream);
}

int hrn_hrnet_backward_in(const void* pk, int dt, int scale, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas,
                          int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, float* d_lrs, float* d_alphas, void* tws,
                          size_t tws_bytes, void* stream) {
    return hrn_hrnet_backward_sel(pk, dt, scale, Pr, alpha_residual, lrs, alphas, B, V, H, W, d_sr, Gr, d_lrs, d_alphas, tws, tws_bytes, stream);
}

// ---- ShiftNet, training: fp32
size_t hrn_shiftnet_train_workspace_bytes(int B) { return hrn_shiftnet_train_workspace_bytes_dt(HRN_DTYPE_F32, B); }

int hrn_shiftnet_forward_train(const void* packed, const hrn_shiftnet_params* P, const float* x, int B, float momentum,
                               const unsigned char* dropout_mask, float* theta, void* tws, size_t tws_bytes, void* stream) {
    return hrn_shiftnet_forward_train_dt(packed, HRN_DTYPE_F32, P, x, B, momentum, dropout_mask, theta, tws, tws_bytes, stream);
}

int hrn_shiftnet_backward(const hrn_shiftnet_params* P, const float* x, int B, const unsigned char* dropout_mask, const float* d_theta,
                          const hrn_shiftnet_params* G, float* d_x, void* tws, size_t tws_bytes, void* stream) {
    return hrn_shiftnet_backward_sel(P, HRN_DTYPE_F32, x, B, dropout_mask, d_theta, G, d_x, tws, tws_bytes, stream);
}

int hrn_shiftnet_backward_dt(const hrn_shiftnet_params* P, int dt, const float* x, int B, const unsigned char* dropout_mask,
                             const float* d_theta, const hrn_shiftnet_params* G, float* d_x, void* tws, size_t tws_bytes, void* stream) {
    return hrn_shiftnet_backward_sel(P, dt, x, B, dropout_mask, d_theta, G, d_x, tws, tws_bytes, stream);
}

// ---- input pipeline: no augmentation codes; scale = 3
int hrn_collate_device_s(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems, const uint8_t* sm_arena,
                         int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale, float* lrs, float* alphas, float* hrs,
                         float* maps, void* stream) {
    return hrn_collate_device_a(lr_arena, lr_elems, hr_arena, hr_elems, sm_arena, sm_elems, plan, B, min_L, S, scale, lrs, alphas, hrs, maps,
                                nullptr, stream);
}
int hrn_collate_device(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems, const uint8_t* sm_arena,
                       int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, float* lrs, float* alphas, float* hrs, float* maps,
                       void* stream) {
    return hrn_collate_device_s(lr_arena, lr_elems, hr_arena, hr_elems, sm_arena, sm_elems, plan, B, min_L, S, 3, lrs, alphas, hrs, maps, stream);
}

}  // extern "C"
