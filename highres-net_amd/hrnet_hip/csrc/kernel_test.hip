// The definitions of the test suite's kernel-level hooks hrn_kt_*; kernel_test.h declares them and states each one's contract.
#include <string.h>
#include "kernel_test.h"
#include "kernels.h"
#include "backward.h"

extern "C" {

size_t hrn_kt_wgrad_scratch_bytes(void) { return hrn_bwd_scratch_bytes(hrn_device_cus()); }

int hrn_kt_conv_wgrad(int dt, const void* x, const void* stack, int pair_h, int pair_last, int pair_vs, const void* g, int M, int H, int W,
                      int cin, int cout, float* dw, void* scratch, void* stream) {
    return hrn_launch_conv_wgrad(dt, x, stack, x ? 0 : 1, pair_h, pair_last, pair_vs, g, M, H, W, cin, cout, dw, scratch, hrn_device_cus(), (hipStream_t)stream);
}

int hrn_kt_conv_dgrad(int dt, int cin, int cout, const float* w, const void* g, void* dx, const void* res, int M, int H, int W, float* wt,
                      void* wtp, const float* zero_bias, void* stream) {
    return hrn_conv_dgrad(dt, cin, cout, w, g, dx, res, M, H, W, wt, wtp, zero_bias, (hipStream_t)stream);
}

int hrn_kt_conv3x3(int dt, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs, const void* wpk,
                   const float* bias, void* out, int M, int H, int W, void* stream) {
    ConvParams p = conv_base(M, H, W);
    p.in = in; p.out = out; p.wpk = wpk; p.bias = bias;
    if (!in) { p.in_pair = 1; p.stack = stack; p.pair_h = pair_h; p.pair_last = pair_last; p.pair_vs = pair_vs; }
    return hrn_launch_conv3x3(dt, cin, cout, p, (hipStream_t)stream, false);
}

// the descriptor of hrn_kt_conv3x3_epi's arguments
static ConvParams epi_params(const void* in, const void* stack, int pair_h, int pair_last, int pair_vs, const void* wpk, const float* bias,
                             const float* slope, const void* res, int res_mode, int res_vs, const float* alphas, int alpha_vs, void* out,
                             int out_h, int out_vs, size_t in_lo, size_t stack_lo, size_t out_lo, size_t res_lo, int M, int H, int W) {
    ConvParams p = conv_base(M, H, W);
    p.in = in; p.in_pair = in ? 0 : 1; p.stack = stack; p.pair_h = pair_h; p.pair_last = pair_last; p.pair_vs = pair_vs;
    p.out = out; p.wpk = wpk; p.bias = bias; p.slope = slope;
    p.res = res; p.res_mode = res_mode; p.res_vs = res_vs; p.alphas = alphas; p.alpha_vs = alpha_vs;
    p.out_h = out_h; p.out_vs = out_vs;
    p.in_lo = in_lo; p.stack_lo = stack_lo; p.out_lo = out_lo; p.res_lo = res_lo;
    return p;
}

int hrn_kt_conv3x3_epi(int dt, int route, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs,
                       const void* wpk, const float* bias, const float* slope, const void* res, int res_mode, int res_vs, const float* alphas,
                       int alpha_vs, void* out, int out_h, int out_vs, size_t in_lo, size_t stack_lo, size_t out_lo, size_t res_lo, int M,
                       int H, int W, void* stream) {
    HRN_CHECK(route == 0 || route == 1, -2, "hrn_kt_conv3x3_epi: route %d", route);
    const ConvParams p = epi_params(in, stack, pair_h, pair_last, pair_vs, wpk, bias, slope, res, res_mode, res_vs, alphas, alpha_vs, out, out_h,
                                    out_vs, in_lo, stack_lo, out_lo, res_lo, M, H, W);
    return hrn_launch_conv3x3(dt, cin, cout, p, (hipStream_t)stream, route == 1);
}

int hrn_kt_conv_route(int dt, int route, int cin, int cout, const void* in, const void* stack, int pair_h, int pair_last, int pair_vs,
                      const void* wpk, const float* bias, const float* slope, const void* res, int res_mode, int res_vs, const float* alphas,
                      int alpha_vs, void* out, int out_h, int out_vs, size_t in_lo, size_t stack_lo, size_t out_lo, size_t res_lo, int M,
                      int H, int W, int in_pair, const float* scale, int relu, const char** family, const char** prof_name, long* grid) {
    HRN_CHECK(route == 0 || route == 1, -2, "hrn_kt_conv_route: route %d", route);
    ConvParams p = epi_params(in, stack, pair_h, pair_last, pair_vs, wpk, bias, slope, res, res_mode, res_vs, alphas, alpha_vs, out, out_h,
                              out_vs, in_lo, stack_lo, out_lo, res_lo, M, H, W);
    p.in_pair = in_pair; p.scale = scale; p.relu = relu;
    ConvRoute r;
    if (const int rc = hrn_conv3x3_route(dt, cin, cout, p, route == 1, r)) return rc;
    static const char* const families[] = {"general", "r64", "v6", "v6x3"};      // ConvFamily
    *family = families[r.family]; *prof_name = r.name; *grid = r.grid;
    return 0;
}

int hrn_kt_stem(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1, const float* sub,
                const float* w, const float* bias, const float* slope, void* out, size_t out_lo, int M, int H, int W, void* stream) {
    return hrn_launch_stem(dt, in0, img_stride0, in1, rep1, img_stride1, sub, w, bias, slope, out, M, H, W, (hipStream_t)stream, out_lo);
}

int hrn_kt_decoder(int dt, int scale, const void* fused, size_t fused_lo, const float* w_iokk, void* wpk, const float* bias,
                   const float* slope, const float* wf, const float* bf, float* sr, int N, int H, int W, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = hrn_launch_decoder_pack(dt == HRN_BF16X3 ? HRN_F32 : dt, w_iokk, wpk, s, scale)) return rc;     // (as api.hip packs it)
    return hrn_launch_decoder(dt, fused, wpk, bias, slope, wf, bf, sr, N, H, W, s, fused_lo, scale);
}

int hrn_kt_conv_pack(int dt, int cin, int cout, const float* w_oihw, void* packed, void* stream) {
    return hrn_launch_conv_pack(dt, cin, cout, w_oihw, packed, (hipStream_t)stream);
}

int hrn_kt_sn_bn_stats(int dt, const void* x, size_t npix, int C, const float* gamma, const float* beta, float* scale, float* shift,
                       float* running_mean, float* running_var, float momentum, double* partial, void* stream) {
    return hrn_launch_bn_stats(dt, x, npix, C, gamma, beta, 1e-5f, scale, shift, running_mean, running_var, momentum, partial, 256,
                               (hipStream_t)stream);
}
int hrn_kt_sn_bn_act_pool(int dt, const void* x, const float* scale, const float* shift, void* out, int N, int H, int W, int C, int pool,
                          void* stream) {
    return hrn_launch_bn_act_pool(dt, x, scale, shift, out, N, H, W, C, pool, (hipStream_t)stream);
}
int hrn_kt_sn_bn_bwd(int dt, const void* x, const void* dy, const float* stats, const float* gamma, void* dx, float* dgamma, float* dbeta,
                     int N, int H, int W, int C, int pool, double* partial, double* sums, void* stream) {
    return hrn_launch_sn_bn_bwd(dt, x, dy, stats, gamma, dx, dgamma, dbeta, N, H, W, C, pool, partial, sums, (hipStream_t)stream);
}
int hrn_kt_sn_stem_dgrad(int dt, const void* g, const float* w, float* din, int M, int H, int W, void* stream) {
    return hrn_launch_sn_stem_dgrad(dt, g, w, din, M, H, W, (hipStream_t)stream);
}
int hrn_kt_sn_fc_to_ref(int dt, const void* y, const unsigned char* mask, float* xr, int B, void* stream) {
    return hrn_launch_fc_to_ref(dt, y, mask, xr, B, (hipStream_t)stream);
}
int hrn_kt_sn_fc_from_ref(int dt, const float* dxr, const unsigned char* mask, void* dy, int B, void* stream) {
    return hrn_launch_fc_from_ref(dt, dxr, mask, dy, B, (hipStream_t)stream);
}

int hrn_kt_sn_bn_save_stats(const double* partial, size_t npix, int C, float* mean, float* invstd, void* stream) {
    return hrn_launch_sn_bn_save_stats(partial, npix, C, 1e-5f, mean, invstd, (hipStream_t)stream);
}
int hrn_kt_sn_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, const float* conv_bias, float* scale,
                      float* shift, int C, void* stream) {
    return hrn_launch_bn_fold(gamma, beta, rm, rv, 1e-5f, conv_bias, scale, shift, C, (hipStream_t)stream);
}
int hrn_kt_sn_conv_bn_relu(int cin, int cout, const float* in, const void* wpk, const float* scale, const float* shift, float* out, int M, int H,
                           int W, void* stream) {
    ConvParams p = conv_base(M, H, W);
    p.in = in; p.out = out;
    p.wpk = wpk; p.scale = scale; p.bias = shift; p.relu = 1;
    return hrn_launch_conv3x3(HRN_F32, cin, cout, p, (hipStream_t)stream, false);
}
int hrn_kt_sn_plane_mean(const float* x, float* mean, int planes, size_t hw, void* stream) {
    return hrn_launch_plane_mean(x, mean, planes, hw, (hipStream_t)stream);
}
int hrn_kt_sn_sub_plane_mean(const float* g, const float* means, float* out, int planes, size_t hw, void* stream) {
    return hrn_launch_sn_sub_plane_mean(g, means, out, planes, hw, (hipStream_t)stream);
}
size_t hrn_kt_sn_fc1_partial_bytes(void) { return hrn_fc1_partial_bytes(); }
int hrn_kt_sn_fc1(const float* xr, const float* w, const float* bias, float* y, int B, float* partial, void* stream) {
    return hrn_launch_fc1(xr, w, bias, y, B, partial, (hipStream_t)stream);
}
int hrn_kt_sn_fc2(const float* y, const float* w2, float* theta, int B, void* stream) {
    return hrn_launch_fc2(y, w2, theta, B, (hipStream_t)stream);
}
int hrn_kt_sn_fc2_bwd(const float* dtheta, const float* y1, const float* w2, float* dz1, float* dw2, float* db1, int B, void* stream) {
    return hrn_launch_sn_fc2_bwd(dtheta, y1, w2, dz1, dw2, db1, B, (hipStream_t)stream);
}
int hrn_kt_sn_fc1_bwd_w(const float* dz1, const float* xr, float* dw1, int B, void* stream) {
    return hrn_launch_sn_fc1_bwd_w(dz1, xr, dw1, B, (hipStream_t)stream);
}
int hrn_kt_sn_fc1_bwd_x(const float* dz1, const float* w1, float* dxr, int B, void* stream) {
    return hrn_launch_sn_fc1_bwd_x(dz1, w1, dxr, B, (hipStream_t)stream);
}

int hrn_kt_prelu_bwd_bias(int dt, const void* dy, const void* y, const void* xpre, const float* slope, void* g, size_t rows, int C,
                          float* dslope, float* db, void* scratch, void* stream) {
    return hrn_launch_prelu_bwd_bias(dt, dy, y, xpre, slope, g, rows, C, dslope, db, scratch, (hipStream_t)stream);
}
int hrn_kt_colsum(int dt, const void* g, size_t rows, int C, float* db, void* scratch, void* stream) {
    return hrn_launch_colsum(dt, g, rows, C, db, scratch, (hipStream_t)stream);
}
int hrn_kt_add(int dt, const void* a, const void* b, void* o, size_t n, void* stream) {
    return hrn_launch_add(dt, a, b, o, n, (hipStream_t)stream);
}
int hrn_kt_fuse_update(int dt, const void* stack, int n_in, const void* f, const float* alphas, int alpha_vs, int pair_last, int half,
                       int alpha_residual, void* out, size_t hw, int B, void* stream) {
    return hrn_launch_fuse_update(dt, stack, n_in, f, alphas, alpha_vs, pair_last, half, alpha_residual, out, hw, B, (hipStream_t)stream);
}
int hrn_kt_pair_add(int dt, const void* stack, int n_in, int half, int pair_last, const void* u, void* t2, size_t hw, int B, void* stream) {
    return hrn_launch_pair_add(dt, stack, n_in, half, pair_last, u, t2, hw, B, (hipStream_t)stream);
}
int hrn_kt_fuse_df(int dt, const void* dsn, const float* alphas, int alpha_vs, int pair_last, int half, int alpha_residual, void* df, size_t hw,
                   int B, void* stream) {
    return hrn_launch_fuse_df(dt, dsn, alphas, alpha_vs, pair_last, half, alpha_residual, df, hw, B, (hipStream_t)stream);
}
int hrn_kt_fuse_scatter(int dt, const void* dsn, const void* dz, int n_in, int half, int pair_last, int alpha_residual, void* ds, size_t hw,
                        int B, void* stream) {
    return hrn_launch_fuse_scatter(dt, dsn, dz, n_in, half, pair_last, alpha_residual, ds, hw, B, (hipStream_t)stream);
}
size_t hrn_kt_alpha_grad_scratch_bytes(int nimg) { return hrn_alpha_grad_scratch_bytes(nimg); }
int hrn_kt_alpha_grad(int dt, const void* dsn, const void* f, int half, int pair_last, float* d_alphas, int B, int V, size_t hw, void* scratch,
                      size_t scratch_bytes, void* stream) {
    return hrn_launch_alpha_grad(dt, dsn, f, half, pair_last, d_alphas, B, V, hw, scratch, scratch_bytes, (hipStream_t)stream);
}
int hrn_kt_stem_wgrad(int dt, const float* in0, size_t stride0, const float* in1, int rep1, size_t stride1, const float* sub, const void* g,
                      int M, int H, int W, float* dw, void* scratch, void* stream) {
    const int cus = hrn_device_cus();
    if (!sub) return hrn_launch_stem_wgrad(dt, in0, stride0, in1, rep1, stride1, g, M, H, W, dw, scratch, cus, (hipStream_t)stream);
    return hrn_launch_stem_wgrad_sub(dt, in0, stride0, in1, rep1, stride1, sub, g, M, H, W, dw, scratch, cus, (hipStream_t)stream);
}
int hrn_kt_stem_dgrad_route(int dt, const void* dA, const float* w, float* wt, const float* lrs, const float* ref, float* d_lrs, int B, int V,
                            int H, int W, void* stream) {
    return hrn_launch_stem_dgrad_route(dt, dA, w, wt, lrs, ref, d_lrs, B, V, H, W, (hipStream_t)stream);
}
int hrn_kt_stem_dgrad_ref(int dt, const void* dA, const float* w, float* wt, float* d_lrs, float* d_ref, int B, int V, int H, int W,
                          void* stream) {
    return hrn_launch_stem_dgrad_ref(dt, dA, w, wt, d_lrs, d_ref, B, V, H, W, (hipStream_t)stream);
}
int hrn_kt_stem_pre(int dt, const float* in0, size_t img_stride0, const float* in1, int rep1, size_t img_stride1, const float* w,
                    const float* bias, void* out, int M, int H, int W, const float* only_if_nonpos, void* stream) {
    return hrn_launch_stem_pre(dt, in0, img_stride0, in1, rep1, img_stride1, w, bias, out, M, H, W, only_if_nonpos, (hipStream_t)stream);
}
int hrn_kt_decoder_bwd(int scale, const float* fused, const float* d_sr, const float* wd, const float* bd, const float* ad, const float* wf,
                       float* d_fused, float* dwd, float* dbd, float* dad, float* dwf, float* dbf, int N, int H, int W, void* scratch,
                       void* stream) {
    return hrn_launch_decoder_bwd(fused, d_sr, wd, bd, ad, wf, d_fused, dwd, dbd, dad, dwf, dbf, N, H, W, scratch, hrn_device_cus(),
                                  (hipStream_t)stream, scale);
}
int hrn_kt_planes_to_f32(const void* hi, size_t lo_off, float* out, size_t n, void* stream) {
    return hrn_launch_planes_to_f32(hi, lo_off, out, n, (hipStream_t)stream);
}
int hrn_kt_f32_to_planes(const float* in, void* hi, size_t lo_off, size_t n, void* stream) {
    return hrn_launch_f32_to_planes(in, hi, lo_off, n, (hipStream_t)stream);
}
int hrn_kt_median(const float* lrs, float* ref, int B, int V, int H, int W, void* stream) {
    return hrn_launch_median(lrs, ref, B, V, H, W, (hipStream_t)stream);
}

}  // extern "C"
