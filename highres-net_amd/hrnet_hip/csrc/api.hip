// extern "C" entry points of libhrnet_hip.so (declared in include/hrnet_hip.h): argument checks, packed-parameter
// and workspace layouts, and the kernel sequences of HRNet.forward / ShiftNet.forward.  (The entry points that are another one with an
// argument fixed are in abi_fixed.hip.)
#include "../../../include/hrnet_hip.h"
#include "kernels.h"
#include "hrnet_layout.h"
#include "shiftnet_layout.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";
void hrn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

namespace {

using namespace hrn;     // packed-parameter layout, at(), conv_site(): hrnet_layout.h

// ---------------------------------------------------------------- HRNet workspace layout
struct HrnetWs {
    size_t ref, emb, buf_a, buf_b, fused, total;
};
HrnetWs hrnet_ws(int dt, int B, int V, int H, int W) {
    HrnetWs w;
    const size_t es = hrn_esize(dt), hw = (size_t)H * W;
    const size_t stack = (size_t)B * V * hw * 64 * es;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = hrn_align_up(off + bytes, ALIGN); return o; };
    w.ref = take((size_t)B * hw * 4);
    w.emb = take(stack);
    w.buf_a = take(stack);      // encoder ping / fusion t1 (B * V/2 images x 128 ch == stack bytes at most)
    w.buf_b = take(stack);      // encoder pong / fusion t2
    w.fused = take((size_t)B * hw * 64 * es);
    w.total = off;
    return w;
}

// HRN_BF16X3: every activation tensor of the workspace is a pair of bf16 planes; the lo plane of the view stack and of the two
// ping-pong buffers starts half a stack further on (a plane of the fusion's 128-channel intermediates is at most that large), the lo
// plane of the fused state B*HW*64 bf16 further on.  0 for the other dtypes.
size_t stack_lo(int dt, int B, int V, int H, int W) { return dt == HRN_BF16X3 ? (size_t)B * V * H * W * 64 * 2 : 0; }
size_t fused_lo(int dt, int B, int H, int W) { return dt == HRN_BF16X3 ? (size_t)B * H * W * 64 * 2 : 0; }
bool dtype_ok(int dt) { return dt == HRN_F32 || dt == HRN_BF16 || dt == HRN_BF16X3; }

int check_scale(int scale) {
    HRN_CHECK(hrn_scale_ok(scale), -2, "scale must be 2, 3 or 4 (decoder kernel_size == stride; got %d)", scale);
    return 0;
}

int check_common(int dt, int nl, int B, int V, int H, int W) {
    HRN_CHECK(dtype_ok(dt), -2, "dtype must be HRN_DTYPE_F32, HRN_DTYPE_BF16 or HRN_DTYPE_BF16X3 (got %d)", dt);
    HRN_CHECK(nl >= 0 && nl <= HRN_MAX_RES_LAYERS, -2, "num_layers %d out of range 0..%d", nl, HRN_MAX_RES_LAYERS);
    HRN_CHECK(B > 0 && V > 0 && H > 0 && W > 0, -2, "empty input B=%d V=%d H=%d W=%d", B, V, H, W);
    return 0;
}

// ext_ref: the reference frame (B,H,W) the stem reads in place of the median of lrs[:, :9] (null: the median, into the workspace's slot)
int encoder_impl(const void* pk, int dt, int nl, const float* lrs, const float* ext_ref, int B, int V, int H, int W,
                 void* emb, void* ws, const HrnetWs& wl, hipStream_t s) {
    const HrnetLayout L = hrnet_layout(dt, nl, 3);        // (the encoder's offsets are the same at every scale)
    const size_t hw = (size_t)H * W;
    const float* ref = ext_ref ? ext_ref : (const float*)at(ws, wl.ref);
    void* bufA = at(ws, wl.buf_a);
    void* bufB = at(ws, wl.buf_b);
    int rc;
    if (!ext_ref && (rc = hrn_launch_median(lrs, (float*)at(ws, wl.ref), B, V, H, W, s))) return rc;
    // stem: channel 0 = view, channel 1 = the sample's reference frame; 2->64 + PReLU  (HRNet.py:200-204, :51-53)
    const size_t lo = stack_lo(dt, B, V, H, W);        // bf16x3: lo plane of bufA / bufB / emb (0 otherwise)
    const ConvSite& stem = L.site[SITE_STEM];
    if ((rc = hrn_launch_stem(dt, lrs, hw, ref, V, hw, nullptr, (const float*)at(pk, stem.w), (const float*)at(pk, stem.b),
                              (const float*)at(pk, stem.a), bufA, B * V, H, W, s, lo))) return rc;
    // residual blocks: A -conv+PReLU-> B -conv+PReLU, + A-> A (in place: the residual is read at the stored pixel only)
    for (int l = 0; l < nl; ++l) {
        ConvParams p = conv_base(B * V, H, W);
        p.in = bufA; p.out = bufB; p.in_lo = p.out_lo = lo;
        conv_site(p, pk, L.site[site_enc(l, 0)]);
        if ((rc = hrn_launch_conv3x3(dt, 64, 64, p, s, false))) return rc;
        ConvParams q = conv_base(B * V, H, W);
        q.in = bufB; q.out = bufA; q.res = bufA; q.res_mode = 1; q.in_lo = q.out_lo = q.res_lo = lo;
        conv_site(q, pk, L.site[site_enc(l, 1)]);
        if ((rc = hrn_launch_conv3x3(dt, 64, 64, q, s, false))) return rc;
    }
    ConvParams f = conv_base(B * V, H, W);
    f.in = bufA; f.out = emb; f.in_lo = f.out_lo = lo;
    conv_site(f, pk, L.site[site_enc_final(nl)]);
    return hrn_launch_conv3x3(dt, 64, 64, f, s, false);
}

int fuse_impl(const void* pk, int dt, int nl, int alpha_residual, void* emb, const float* alphas, int B, int V, int H, int W,
              void* fused, void* ws, const HrnetWs& wl, hipStream_t s) {
    const HrnetLayout L = hrnet_layout(dt, nl, 3);        // (the fusion's offsets are the same at every scale)
    const size_t hw = (size_t)H * W, es = hrn_esize(dt);
    void* t1 = at(ws, wl.buf_a);
    void* t2 = at(ws, wl.buf_b);
    const size_t lo = stack_lo(dt, B, V, H, W), flo = fused_lo(dt, B, H, W);
    int n = V, rc;
    if (n / 2 == 0) {   // V == 1: no fusion level; mean over one view is the identity (HRNet.py:113,134)
        HRN_HIP(hipMemcpyAsync(fused, emb, (size_t)B * hw * 64 * es, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    while (n / 2 > 0) {
        const int parity = n & 1, half = n >> 1;
        const bool last = (half == 1);
        // g: z = cat(s_i, s_partner) -> t1 = PReLU(conv(z))                 (ResidualBlock first half, HRNet.py:18-19)
        ConvParams a = conv_base(B * half, H, W);
        a.in_pair = 1; a.stack = emb; a.pair_h = half; a.pair_last = n - parity - 1; a.pair_vs = V;
        a.out = t1; a.stack_lo = a.out_lo = lo;
        conv_site(a, pk, L.site[site_fres(nl, 0)]);
        if ((rc = hrn_launch_conv3x3(dt, 128, 128, a, s, false))) return rc;
        // t2 = z + PReLU(conv(t1))                                          (HRNet.py:20-21, :33)
        ConvParams b = conv_base(B * half, H, W);
        b.in = t1; b.out = t2; b.in_lo = b.out_lo = b.stack_lo = lo;
        b.res_mode = 2;      // residual = the same pair gather, straight from the stack
        b.stack = emb; b.pair_h = half; b.pair_last = n - parity - 1; b.pair_vs = V;
        conv_site(b, pk, L.site[site_fres(nl, 1)]);
        if ((rc = hrn_launch_conv3x3(dt, 128, 128, b, s, false))) return rc;
        // f = PReLU(conv(t2)); s_i <- s_i + alpha_partner * f  (or s_i <- f)  (HRNet.py:95-97, :123-128)
        ConvParams c = conv_base(B * half, H, W);
        c.in = t2; c.in_lo = c.res_lo = lo;
        c.out_h = half;
        if (last) { c.out = fused; c.out_vs = 1; c.out_lo = flo; } else { c.out = emb; c.out_vs = V; c.out_lo = lo; }
        c.pair_last = n - parity - 1;
        if (alpha_residual) { c.res_mode = 3; c.res = emb; c.res_vs = V; c.alphas = alphas; c.alpha_vs = V; }
        conv_site(c, pk, L.site[site_fout(nl)]);
        if ((rc = hrn_launch_conv3x3(dt, 128, 64, c, s, false))) return rc;
        n = half;
    }
    return 0;
}

int decoder_impl(const void* pk, int dt, int nl, int scale, const void* fused, int N, int H, int W, float* sr, hipStream_t s) {
    const HrnetLayout L = hrnet_layout(dt, nl, scale);
    return hrn_launch_decoder(dt, fused, at(pk, L.dec_w), (const float*)at(pk, L.dec_b), (const float*)at(pk, L.dec_a),
                              (const float*)at(pk, L.fin_w), (const float*)at(pk, L.fin_b), sr, N, H, W, s, fused_lo(dt, N, H, W), scale);
}

// ---------------------------------------------------------------- ShiftNet layouts (packed parameters: shiftnet_layout.h)
struct SnWs {
    size_t means, scale, shift, partial, x, y, fc, xr, fc_partial, total;
};
SnWs sn_ws(int B) {
    SnWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = hrn_align_up(off + bytes, ALIGN); return o; };
    w.means = take((size_t)B * 2 * 4);
    w.scale = take(128 * 4); w.shift = take(128 * 4);
    w.partial = take((size_t)SN_PARTIAL_BLOCKS * 128 * 2 * 8);
    w.x = take((size_t)B * 128 * 128 * 64 * 4);     // conv output (pre-BN), largest at layer 1/2
    w.y = take((size_t)B * 128 * 128 * 64 * 4);     // activation after BN+ReLU(+pool)
    w.fc = take((size_t)B * 1024 * 4);
    w.xr = take((size_t)B * 32768 * 4);             // fc1's input in the reference's flatten order
    w.fc_partial = take(hrn_fc1_partial_bytes());
    w.total = off;
    return w;
}

}  // namespace

// ================================================================= C ABI
extern "C" {

int hrn_version(void) { return HRN_ABI_VERSION; }
const char* hrn_last_error(void) { return g_err; }

size_t hrn_hrnet_packed_bytes_s(int dtype, int num_layers, int scale) {
    if (!dtype_ok(dtype) || num_layers < 0 || num_layers > HRN_MAX_RES_LAYERS || !hrn_scale_ok(scale)) return 0;
    return hrnet_layout(dtype, num_layers, scale).total;
}

int hrn_hrnet_pack_s(const hrn_hrnet_params* P, int dt, int scale, void* packed, size_t packed_bytes, void* stream) {
    int rc;
    if ((rc = check_scale(scale))) return rc;
    HRN_CHECK(P && packed, -2, "hrn_hrnet_pack: null argument");
    if ((rc = check_common(dt, P->num_layers, 1, 1, 1, 1))) return rc;
    const int nl = P->num_layers;
    const HrnetLayout L = hrnet_layout(dt, nl, scale);
    HRN_CHECK(packed_bytes >= L.total, -3, "hrn_hrnet_pack: packed buffer too small (%zu < %zu)", packed_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    auto copy = [&](size_t off, const float* src, size_t n) -> int {
        HRN_CHECK(src != nullptr, -2, "hrn_hrnet_pack: null parameter pointer");
        HRN_HIP(hipMemcpyAsync(at(packed, off), src, n * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    for (int k = 0; k < num_sites(nl); ++k) {
        const ConvSite& c = L.site[k];
        const SiteParams p = site_params(P, nl, k);
        if (k == SITE_STEM) {               // the stem kernel reads the raw f32 weights
            if ((rc = copy(c.w, p.w, 64 * 18))) return rc;
        } else {
            if (k < site_enc_final(nl)) HRN_CHECK(p.w, -2, "hrn_hrnet_pack: null encoder weight %d", k - site_enc(0, 0));
            else if (k == site_fres(nl, 0) || k == site_fres(nl, 1)) HRN_CHECK(p.w, -2, "hrn_hrnet_pack: null fuse weight %d", k - site_fres(nl, 0));
            else HRN_CHECK(p.w, -2, "hrn_hrnet_pack: null weight pointer");
            if ((rc = hrn_launch_conv_pack(dt, c.cin, c.cout, p.w, at(packed, c.w), s))) return rc;
        }
        if ((rc = copy(c.b, p.b, c.cout)) || (c.prelu && (rc = copy(c.a, p.a, 1)))) return rc;
    }
    HRN_CHECK(P->dec_w, -2, "hrn_hrnet_pack: null weight pointer");
    if ((rc = hrn_launch_decoder_pack(dt == HRN_BF16X3 ? HRN_F32 : dt, P->dec_w, at(packed, L.dec_w), s, scale))) return rc;     // bf16x3: the decoder is the fp32 one
    if ((rc = copy(L.dec_b, P->dec_b, 64)) || (rc = copy(L.dec_a, P->dec_a, 1))) return rc;
    if ((rc = copy(L.fin_w, P->fin_w, 64)) || (rc = copy(L.fin_b, P->fin_b, 1))) return rc;
    return 0;
}

size_t hrn_hrnet_workspace_bytes(int dtype, int B, int V, int H, int W) {
    if (!dtype_ok(dtype) || B <= 0 || V <= 0 || H <= 0 || W <= 0) return 0;
    return hrnet_ws(dtype, B, V, H, W).total;
}

int hrn_encoder_forward(const void* packed, int dt, int nl, const float* lrs, int B, int V, int H, int W,
                        void* emb, void* ws, size_t ws_bytes, void* stream) {
    int rc;
    if ((rc = check_common(dt, nl, B, V, H, W))) return rc;
    HRN_CHECK(packed && lrs && emb && ws, -2, "hrn_encoder_forward: null argument");
    const HrnetWs wl = hrnet_ws(dt, B, V, H, W);
    HRN_CHECK(ws_bytes >= wl.total, -3, "hrn_encoder_forward: workspace too small (%zu < %zu)", ws_bytes, wl.total);
    return encoder_impl(packed, dt, nl, lrs, nullptr, B, V, H, W, emb, ws, wl, (hipStream_t)stream);
}

int hrn_fuse_forward(const void* packed, int dt, int nl, int alpha_residual, void* emb, const float* alphas,
                     int B, int V, int H, int W, void* fused, void* ws, size_t ws_bytes, void* stream) {
    int rc;
    if ((rc = check_common(dt, nl, B, V, H, W))) return rc;
    HRN_CHECK(packed && emb && alphas && fused && ws, -2, "hrn_fuse_forward: null argument");
    const HrnetWs wl = hrnet_ws(dt, B, V, H, W);
    HRN_CHECK(ws_bytes >= wl.total, -3, "hrn_fuse_forward: workspace too small (%zu < %zu)", ws_bytes, wl.total);
    return fuse_impl(packed, dt, nl, alpha_residual, emb, alphas, B, V, H, W, fused, ws, wl, (hipStream_t)stream);
}

int hrn_decoder_forward_s(const void* packed, int dt, int nl, int scale, const void* fused, int N, int H, int W, float* sr, void* stream) {
    int rc;
    if ((rc = check_scale(scale)) || (rc = check_common(dt, nl, N, 1, H, W))) return rc;
    HRN_CHECK(packed && fused && sr, -2, "hrn_decoder_forward: null argument");
    return decoder_impl(packed, dt, nl, scale, fused, N, H, W, sr, (hipStream_t)stream);
}

static int hrnet_forward_impl(const void* packed, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas,
                              const float* ext_ref, int B, int V, int H, int W, float* sr, void* ws, size_t ws_bytes, void* stream) {
    int rc;
    if ((rc = check_scale(scale)) || (rc = check_common(dt, nl, B, V, H, W))) return rc;
    HRN_CHECK(packed && lrs && alphas && sr && ws, -2, "hrn_hrnet_forward: null argument");
    const HrnetWs wl = hrnet_ws(dt, B, V, H, W);
    HRN_CHECK(ws_bytes >= wl.total, -3, "hrn_hrnet_forward: workspace too small (%zu < %zu)", ws_bytes, wl.total);
    hipStream_t s = (hipStream_t)stream;
    void* emb = at(ws, wl.emb);
    void* fused = at(ws, wl.fused);
    if ((rc = encoder_impl(packed, dt, nl, lrs, ext_ref, B, V, H, W, emb, ws, wl, s))) return rc;
    if ((rc = fuse_impl(packed, dt, nl, alpha_residual, emb, alphas, B, V, H, W, fused, ws, wl, s))) return rc;
    return decoder_impl(packed, dt, nl, scale, fused, B, H, W, sr, s);
}

int hrn_hrnet_forward_s(const void* packed, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas,
                        int B, int V, int H, int W, float* sr, void* ws, size_t ws_bytes, void* stream) {
    return hrnet_forward_impl(packed, dt, nl, scale, alpha_residual, lrs, alphas, nullptr, B, V, H, W, sr, ws, ws_bytes, stream);
}

int hrn_hrnet_forward_ref(const void* packed, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas,
                          const float* ref, int B, int V, int H, int W, float* sr, void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(ref, -2, "hrn_hrnet_forward_ref: null argument (ref)");
    return hrnet_forward_impl(packed, dt, nl, scale, alpha_residual, lrs, alphas, ref, B, V, H, W, sr, ws, ws_bytes, stream);
}

// ----------------------------------------------------------------- ShiftNet
size_t hrn_shiftnet_packed_bytes(void) { return sn_layout().total; }

int hrn_shiftnet_pack(const hrn_shiftnet_params* P, void* packed, size_t packed_bytes, void* stream) {
    HRN_CHECK(P && packed, -2, "hrn_shiftnet_pack: null argument");
    const SnLayout L = sn_layout();
    HRN_CHECK(packed_bytes >= L.total, -3, "hrn_shiftnet_pack: packed buffer too small (%zu < %zu)", packed_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    for (int i = 0; i < 8; ++i) {
        HRN_CHECK(P->conv_w[i] && P->conv_b[i], -2, "hrn_shiftnet_pack: null conv parameter %d", i);
        if (i == 0) {
            HRN_HIP(hipMemcpyAsync(at(packed, L.conv_w[0]), P->conv_w[0], 64 * 18 * 4, hipMemcpyDeviceToDevice, s));
        } else if ((rc = hrn_launch_conv_pack(HRN_F32, SN_CI[i], SN_CO[i], P->conv_w[i], at(packed, L.conv_w[i]), s))) {
            return rc;
        }
        HRN_HIP(hipMemcpyAsync(at(packed, L.conv_b[i]), P->conv_b[i], SN_CO[i] * 4, hipMemcpyDeviceToDevice, s));
    }
    HRN_CHECK(P->fc1_b && P->fc2_w, -2, "hrn_shiftnet_pack: null fc parameter");
    HRN_HIP(hipMemcpyAsync(at(packed, L.fc1_b), P->fc1_b, 1024 * 4, hipMemcpyDeviceToDevice, s));
    HRN_HIP(hipMemcpyAsync(at(packed, L.fc2_w), P->fc2_w, 2 * 1024 * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

size_t hrn_shiftnet_workspace_bytes(int B) { return B > 0 ? sn_ws(B).total : 0; }

int hrn_shiftnet_forward(const void* packed, const hrn_shiftnet_params* P, const float* x, int B, int train_bn, float momentum,
                         const unsigned char* dropout_mask, float* theta, void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(packed && P && x && theta && ws, -2, "hrn_shiftnet_forward: null argument");
    HRN_CHECK(P->fc1_w, -2, "hrn_shiftnet_forward: params->fc1_w is null (fc1.weight is read in place)");
    HRN_CHECK(B > 0, -2, "hrn_shiftnet_forward: empty batch");
    const SnLayout L = sn_layout();
    const SnWs wl = sn_ws(B);
    HRN_CHECK(ws_bytes >= wl.total, -3, "hrn_shiftnet_forward: workspace too small (%zu < %zu)", ws_bytes, wl.total);
    hipStream_t s = (hipStream_t)stream;
    float* means = (float*)at(ws, wl.means);
    float* scale = (float*)at(ws, wl.scale);
    float* shift = (float*)at(ws, wl.shift);
    double* partial = (double*)at(ws, wl.partial);
    float* bx = (float*)at(ws, wl.x);
    float* by = (float*)at(ws, wl.y);
    float* fc = (float*)at(ws, wl.fc);
    int rc, hsz = 128;
    const size_t plane = 128 * 128;
    if ((rc = hrn_launch_plane_mean(x, means, B * 2, plane, s))) return rc;                      // ShiftNet.py:58
    for (int i = 0; i < 8; ++i) {
        HRN_CHECK(P->bn_g[i] && P->bn_b[i] && P->bn_rm[i] && P->bn_rv[i], -2, "hrn_shiftnet_forward: null BatchNorm tensor %d", i);
        const int C = SN_CO[i];
        if (i > 0 && !train_bn) {
            // eval mode: BatchNorm (running statistics) + ReLU are the convolution's epilogue - one launch per layer instead of three and
            // no pre-BatchNorm tensor; the pooled layers keep a pool-only pass                         ShiftNet.py:16-42 in .eval()
            if ((rc = hrn_launch_bn_fold(P->bn_g[i], P->bn_b[i], P->bn_rm[i], P->bn_rv[i], 1e-5f, (const float*)at(packed, L.conv_b[i]),
                                         scale, shift, C, s))) return rc;
            ConvParams p = conv_base(B, hsz, hsz);
            p.in = by; p.out = bx;
            p.wpk = at(packed, L.conv_w[i]); p.scale = scale; p.bias = shift; p.relu = 1;
            if ((rc = hrn_launch_conv3x3(HRN_F32, SN_CI[i], C, p, s, false))) return rc;
            if (SN_POOL[i]) {
                if ((rc = hrn_launch_bn_act_pool(HRN_F32, bx, nullptr, nullptr, by, B, hsz, hsz, C, 1, s))) return rc;
                hsz /= 2;
            } else {
                float* t = bx; bx = by; by = t;             // the activation is where the conv wrote it
            }
            continue;
        }
        if (i == 0) {
            if ((rc = hrn_launch_stem(HRN_F32, x, 2 * plane, x + plane, 1, 2 * plane, means, (const float*)at(packed, L.conv_w[0]),
                                      (const float*)at(packed, L.conv_b[0]), nullptr, bx, B, hsz, hsz, s, 0))) return rc;
        } else {
            ConvParams p = conv_base(B, hsz, hsz);
            p.in = by; p.out = bx;
            p.wpk = at(packed, L.conv_w[i]); p.bias = (const float*)at(packed, L.conv_b[i]);
            if ((rc = hrn_launch_conv3x3(HRN_F32, SN_CI[i], SN_CO[i], p, s, false))) return rc;
        }
        if (train_bn) {
            if ((rc = hrn_launch_bn_stats(HRN_F32, bx, (size_t)B * hsz * hsz, C, P->bn_g[i], P->bn_b[i], 1e-5f, scale, shift,
                                          P->bn_rm[i], P->bn_rv[i], momentum, partial, SN_PARTIAL_BLOCKS, s))) return rc;
        } else {
            if ((rc = hrn_launch_bn_fold(P->bn_g[i], P->bn_b[i], P->bn_rm[i], P->bn_rv[i], 1e-5f, nullptr, scale, shift, C, s))) return rc;
        }
        if ((rc = hrn_launch_bn_act_pool(HRN_F32, bx, scale, shift, by, B, hsz, hsz, C, SN_POOL[i], s))) return rc;
        if (SN_POOL[i]) hsz /= 2;
    }
    // by: [B][16][16][128] NHWC -> xr [B][c*256 + hw], the reference's flatten order (dropout folded in); fc1.weight is read in place
    float* xr = (float*)at(ws, wl.xr);
    if ((rc = hrn_launch_fc_to_ref(HRN_F32, by, dropout_mask, xr, B, s))) return rc;
    if ((rc = hrn_launch_fc1(xr, P->fc1_w, (const float*)at(packed, L.fc1_b), fc, B, (float*)at(ws, wl.fc_partial), s))) return rc;
    return hrn_launch_fc2(fc, (const float*)at(packed, L.fc2_w), theta, B, s);
}

// ----------------------------------------------------------------- Lanczos
int hrn_lanczos_kernel(const float* dx, int n, float* taps, void* stream) {
    HRN_CHECK(n >= 0 && (n == 0 || (dx && taps)), -2, "hrn_lanczos_kernel: bad argument");
    return hrn_launch_lanczos_taps(dx, n, taps, (hipStream_t)stream);
}

int hrn_lanczos_shift(const float* img, const float* shift, int b, int c, int H, int W, float* out, void* stream) {
    HRN_CHECK(b >= 0 && c >= 0 && H > 0 && W > 0, -2, "hrn_lanczos_shift: bad shape");
    HRN_CHECK(b * c == 0 || (img && shift && out), -2, "hrn_lanczos_shift: null argument");
    return hrn_launch_lanczos_shift(img, shift, b, c, H, W, out, (hipStream_t)stream);
}

// ----------------------------------------------------------------- loss / score reductions
size_t hrn_lanczos_shift_backward_workspace_bytes(int b, int c, int H, int W) {
    if (b <= 0 || c <= 0 || H <= 0 || W <= 0) return 0;
    return hrn_lanczos_bwd_workspace_bytes_impl(b, c, H, W);
}

int hrn_lanczos_shift_backward(const float* img, const float* shift, const float* d_out, int b, int c, int H, int W, float* d_img,
                               float* d_shift, void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(img && shift && d_out && ws, -2, "hrn_lanczos_shift_backward: null argument");
    HRN_CHECK(b > 0 && c > 0, -2, "hrn_lanczos_shift_backward: empty input b=%d c=%d", b, c);
    HRN_CHECK(ws_bytes >= hrn_lanczos_bwd_workspace_bytes_impl(b, c, H, W), -3, "hrn_lanczos_shift_backward: workspace too small");
    return hrn_launch_lanczos_shift_bwd(img, shift, d_out, b, c, H, W, d_img, d_shift, ws, (hipStream_t)stream);
}

int hrn_get_loss(const float* srs, const float* hrs, const float* maps, int B, int S, int crop, int metric, float* out, void* stream) {
    HRN_CHECK(B > 0 && S > 0 && crop >= 0 && 2 * crop < S, -2, "hrn_get_loss: bad shape B=%d S=%d crop=%d", B, S, crop);
    HRN_CHECK(metric >= 0 && metric <= 2, -2, "hrn_get_loss: metric must be 0 (masked_MSE), 1 (cMSE) or 2 (cPSNR)");
    HRN_CHECK(srs && hrs && maps && out, -2, "hrn_get_loss: null argument");
    return hrn_launch_masked_cmse(srs, hrs, maps, B, S, crop, metric, out, (hipStream_t)stream);
}

size_t hrn_get_loss_train_workspace_bytes(int B) { return B > 0 ? hrn_loss_train_workspace_bytes_impl(B) : 0; }

int hrn_get_loss_train(const float* srs, const float* hrs, const float* maps, int B, int S, int crop, int metric, float* out,
                       double* stats, void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(B > 0 && B <= 65535 && S > 0 && crop >= 0 && 2 * crop < S, -2, "hrn_get_loss_train: bad shape B=%d S=%d crop=%d", B, S, crop);
    HRN_CHECK(metric == 1 || metric == 2, -2, "hrn_get_loss_train: metric must be 1 (cMSE) or 2 (cPSNR); masked_MSE has no registered form");
    HRN_CHECK(srs && hrs && maps && out && stats && ws, -2, "hrn_get_loss_train: null argument");
    HRN_CHECK(ws_bytes >= hrn_loss_train_workspace_bytes_impl(B), -3, "hrn_get_loss_train: workspace too small");
    return hrn_launch_loss_train(srs, hrs, maps, B, S, crop, metric, out, stats, (double*)ws, (hipStream_t)stream);
}

int hrn_get_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B, int S,
                          int crop, int metric, float* d_srs, void* stream) {
    HRN_CHECK(B > 0 && B <= 65535 && S > 0 && crop >= 0 && 2 * crop < S, -2, "hrn_get_loss_backward: bad shape B=%d S=%d crop=%d", B, S, crop);
    HRN_CHECK(metric == 1 || metric == 2, -2, "hrn_get_loss_backward: metric must be 1 (cMSE) or 2 (cPSNR)");
    HRN_CHECK(srs && hrs && maps && stats && d_out && d_srs, -2, "hrn_get_loss_backward: null argument");
    return hrn_launch_loss_backward(srs, hrs, maps, stats, d_out, B, S, crop, metric, d_srs, (hipStream_t)stream);
}

size_t hrn_shift_cpsnr_workspace_bytes(int B, int border) {
    if (B <= 0 || border < 0) return 0;
    return (size_t)B * (2 * border + 1) * (2 * border + 1) * sizeof(double);
}

int hrn_shift_cpsnr(const float* srs, const float* hrs, const float* maps, int B, int S, int border, int clip, float* out,
                    void* ws, size_t ws_bytes, void* stream) {
    HRN_CHECK(B > 0 && border >= 0 && S > 2 * border, -2, "hrn_shift_cpsnr: bad shape B=%d S=%d border=%d", B, S, border);
    HRN_CHECK(B <= 65535, -2, "hrn_shift_cpsnr: batch %d exceeds the grid limit", B);
    HRN_CHECK(srs && hrs && maps && out && ws, -2, "hrn_shift_cpsnr: null argument");
    HRN_CHECK(ws_bytes >= hrn_shift_cpsnr_workspace_bytes(B, border), -3, "hrn_shift_cpsnr: workspace too small");
    return hrn_launch_shift_cpsnr(srs, hrs, maps, B, S, border, clip, (double*)ws, out, (hipStream_t)stream);
}

// shift_cPSNR's offset search (Evaluator.py:52-73) over get_loss's cMSE (train.py:66-87), differentiable, frames of any aspect ratio
static int shift_loss_check(const char* who, int B, int H, int W, int border, int metric) {
    HRN_CHECK(border >= 0 && border <= 8, -2, "%s: border %d outside 0..8", who, border);
    HRN_CHECK(B > 0 && H > 2 * border && W > 2 * border, -2, "%s: bad shape B=%d H=%d W=%d border=%d", who, B, H, W, border);
    HRN_CHECK(B <= 65535, -2, "%s: batch %d exceeds the grid limit", who, B);
    HRN_CHECK(metric == 1 || metric == 2, -2, "%s: metric must be 1 (cMSE) or 2 (cPSNR); masked_MSE has no searched form", who);
    return 0;
}

size_t hrn_shift_loss_workspace_bytes(int B, int H, int W, int border) {
    if (B <= 0 || border < 0 || border > 8 || H <= 2 * border || W <= 2 * border) return 0;
    return hrn_shift_loss_workspace_bytes_impl(B, H, W, border);
}

// Evaluator.py:52-73 and train.py:66-87: the forward of the searched loss
int hrn_shift_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int metric, int clip,
                         float* out, double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = shift_loss_check("hrn_shift_loss_train", B, H, W, border, metric)) return rc;
    HRN_CHECK(srs && hrs && maps && out && stats && ws, -2, "hrn_shift_loss_train: null argument");
    HRN_CHECK(ws_bytes >= hrn_shift_loss_workspace_bytes_impl(B, H, W, border), -3, "hrn_shift_loss_train: workspace too small");
    return hrn_launch_shift_loss_train(srs, hrs, maps, B, H, W, border, metric, clip != 0, out, stats, (double*)ws, (hipStream_t)stream);
}

// Evaluator.py:52-73 and train.py:66-87: its backward, through the selected offset
int hrn_shift_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B, int H,
                            int W, int border, int metric, int clip, float* d_srs, void* stream) {
    if (int rc = shift_loss_check("hrn_shift_loss_backward", B, H, W, border, metric)) return rc;
    HRN_CHECK(srs && hrs && maps && stats && d_out && d_srs, -2, "hrn_shift_loss_backward: null argument");
    return hrn_launch_shift_loss_backward(srs, hrs, maps, stats, d_out, B, H, W, border, metric, clip != 0, d_srs, (hipStream_t)stream);
}

// the shift-searched SSIM (cssim.hip): the same crops and offsets, no gradient
static int shift_cssim_check(const char* who, int B, int H, int W, int border, int window) {
    HRN_CHECK(border >= 0 && border <= 8, -2, "%s: border %d outside 0..8", who, border);
    HRN_CHECK(window == 0 || window == 1, -2, "%s: window must be 0 (gaussian, 11 taps) or 1 (uniform, 7 taps); got %d", who, window);
    const int side = 2 * border + (window == 1 ? 7 : 11);
    HRN_CHECK(B > 0 && H >= side && W >= side, -2, "%s: bad shape B=%d H=%d W=%d: a side must be at least 2 border + taps = %d", who, B, H, W,
              side);
    HRN_CHECK(B <= 65535, -2, "%s: batch %d exceeds the grid limit", who, B);
    return 0;
}

size_t hrn_shift_cssim_workspace_bytes(int B, int H, int W, int border, int window) {
    if (border < 0 || border > 8 || (window != 0 && window != 1)) return 0;
    const int side = 2 * border + (window == 1 ? 7 : 11);
    if (B <= 0 || B > 65535 || H < side || W < side) return 0;
    return hrn_shift_cssim_workspace_bytes_impl(B, H, W, border, window);
}

int hrn_shift_cssim(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int window, int clip,
                    int correct_bias, float data_range, float* out, double* stats, double* scores, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = shift_cssim_check("hrn_shift_cssim", B, H, W, border, window)) return rc;
    HRN_CHECK(data_range > 0.f && data_range <= 3.0e38f, -2, "hrn_shift_cssim: data_range must be positive and finite (got %g)", (double)data_range);
    HRN_CHECK(srs && hrs && maps && out && stats && ws, -2, "hrn_shift_cssim: null argument");
    HRN_CHECK(ws_bytes >= hrn_shift_cssim_workspace_bytes_impl(B, H, W, border, window), -3, "hrn_shift_cssim: workspace too small");
    return hrn_launch_shift_cssim(srs, hrs, maps, B, H, W, border, window, clip != 0, correct_bias != 0, data_range, out, stats, scores, ws,
                                  (hipStream_t)stream);
}

// cSSIM as a loss (cssim_bwd.hip): the gradient through the offset the forward selected
size_t hrn_cssim_loss_backward_workspace_bytes(int B, int H, int W, int border, int window) {
    if (hrn_shift_cssim_workspace_bytes(B, H, W, border, window) == 0) return 0;       // the same arguments are refused
    return hrn_cssim_loss_backward_workspace_bytes_impl(B, H, W, border, window);
}

int hrn_cssim_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B, int H,
                            int W, int border, int window, int clip, int correct_bias, float data_range, float* d_srs, void* ws,
                            size_t ws_bytes, void* stream) {
    if (int rc = shift_cssim_check("hrn_cssim_loss_backward", B, H, W, border, window)) return rc;
    HRN_CHECK(data_range > 0.f && data_range <= 3.0e38f, -2, "hrn_cssim_loss_backward: data_range must be positive and finite (got %g)",
              (double)data_range);
    HRN_CHECK(srs && hrs && maps && stats && d_out && d_srs && ws, -2, "hrn_cssim_loss_backward: null argument");
    HRN_CHECK(ws_bytes >= hrn_cssim_loss_backward_workspace_bytes_impl(B, H, W, border, window), -3,
              "hrn_cssim_loss_backward: workspace too small");
    return hrn_launch_cssim_loss_backward(srs, hrs, maps, stats, d_out, B, H, W, border, window, clip != 0, correct_bias != 0, data_range,
                                          d_srs, ws, (hipStream_t)stream);
}

// the shift-searched L1 / Charbonnier (cl1_loss.hip): shift_loss's crops, offsets and limits
static int cl1_loss_check(const char* who, int B, int H, int W, int border, float eps) {
    HRN_CHECK(border >= 0 && border <= 8, -2, "%s: border %d outside 0..8", who, border);
    HRN_CHECK(B > 0 && H > 2 * border && W > 2 * border, -2, "%s: bad shape B=%d H=%d W=%d border=%d", who, B, H, W, border);
    HRN_CHECK(B <= 65535, -2, "%s: batch %d exceeds the grid limit", who, B);
    HRN_CHECK((long long)H * W <= 0x7fffffffLL, -2, "%s: a frame of %d x %d exceeds 2^31 - 1 pixels", who, H, W);
    HRN_CHECK(eps >= 0.f && eps <= 3.0e38f, -2, "%s: eps must be finite and not negative (got %g)", who, (double)eps);
    return 0;
}

size_t hrn_cl1_loss_workspace_bytes(int B, int H, int W, int border) {
    if (B <= 0 || B > 65535 || border < 0 || border > 8 || H <= 2 * border || W <= 2 * border || (long long)H * W > 0x7fffffffLL) return 0;
    return hrn_cl1_loss_workspace_bytes_impl(B, H, W, border);
}

int hrn_cl1_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, float eps, float* out,
                       double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = cl1_loss_check("hrn_cl1_loss_train", B, H, W, border, eps)) return rc;
    HRN_CHECK(srs && hrs && maps && out && stats && ws, -2, "hrn_cl1_loss_train: null argument");
    HRN_CHECK(ws_bytes >= hrn_cl1_loss_workspace_bytes_impl(B, H, W, border), -3, "hrn_cl1_loss_train: workspace too small");
    return hrn_launch_cl1_loss_train(srs, hrs, maps, B, H, W, border, clip != 0, eps, out, stats, (double*)ws, (hipStream_t)stream);
}

int hrn_cl1_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B, int H, int W,
                          int border, int clip, float eps, float* d_srs, void* stream) {
    if (int rc = cl1_loss_check("hrn_cl1_loss_backward", B, H, W, border, eps)) return rc;
    HRN_CHECK(srs && hrs && maps && stats && d_out && d_srs, -2, "hrn_cl1_loss_backward: null argument");
    return hrn_launch_cl1_loss_backward(srs, hrs, maps, stats, d_out, B, H, W, border, clip != 0, eps, d_srs, (hipStream_t)stream);
}

// the masked-NCC registration search (registration.hip): the reference fork's recursive_mncc_search / compute_grid_mncc, restated
//
// Every limit of a registration problem is stated once, in a check that takes the entry point's name `who`.  A size query runs its entry
// point's own checks with a null `who` - which refuses without touching hrn_last_error - and answers 0 where they refuse.
#define MNCC_LIMIT(cond, ...)                                             \
    do {                                                                  \
        if (!(cond)) { if (who) hrn_set_error(__VA_ARGS__); return -2; } \
    } while (0)

static int mncc_check(const char* who, int B, int V, int H, int W, int lo = HRN_MNCC_MIN_SIDE, int hi = HRN_MNCC_MAX_SIDE) {
    MNCC_LIMIT(B > 0 && V > 0 && (long)B * V <= 0x7fffffffL, "%s: bad batch B=%d V=%d", who, B, V);
    MNCC_LIMIT(H >= lo && H <= hi && W >= lo && W <= hi, "%s: bad shape H=%d W=%d: the sides of a frame must be %d..%d", who, H, W, lo, hi);
    return 0;
}

static int mncc_check_points(const char* who, int P) {
    MNCC_LIMIT(P >= HRN_MNCC_MIN_POINTS && P <= HRN_MNCC_MAX_POINTS, "%s: points per axis P=%d outside %d..%d", who, P, HRN_MNCC_MIN_POINTS,
               HRN_MNCC_MAX_POINTS);
    return 0;
}

static int mncc_check_levels(const char* who, const char* name, int levels) {
    MNCC_LIMIT(levels >= 1 && levels <= HRN_MNCC_MAX_LEVELS, "%s: %s %d outside 1..%d", who, name, levels, HRN_MNCC_MAX_LEVELS);
    return 0;
}

static int mncc_check_radius(const char* who, const char* name, float radius) {
    MNCC_LIMIT(radius > 0.f && radius <= 4.f, "%s: %s %g outside (0, 4]", who, name, (double)radius);
    return 0;
}

// points, levels, radius: what every search checks after its shape
static int mncc_check_search(const char* who, int P, int levels, float radius) {
    if (int rc = mncc_check_points(who, P)) return rc;
    if (int rc = mncc_check_levels(who, "levels", levels)) return rc;
    return mncc_check_radius(who, "radius", radius);
}

int hrn_mncc_grid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B, int V,
                  int H, int W, int P, float width, float* scores, void* stream) {
    if (int rc = mncc_check("hrn_mncc_grid", B, V, H, W)) return rc;
    if (int rc = mncc_check_points("hrn_mncc_grid", P)) return rc;
    HRN_CHECK(width > 0.f && width <= 8.f, -2, "hrn_mncc_grid: width %g outside (0, 8]", (double)width);
    HRN_CHECK(ref && views && centres && scores, -2, "hrn_mncc_grid: null argument");
    return hrn_launch_mncc_grid(ref, ref_mask, views, view_masks, centres, B, V, H, W, P, width, scores, (hipStream_t)stream);
}

int hrn_mncc_search(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W, int P,
                    int levels, float radius, float* shifts, float* trace, void* stream) {
    if (int rc = mncc_check("hrn_mncc_search", B, V, H, W)) return rc;
    if (int rc = mncc_check_search("hrn_mncc_search", P, levels, radius)) return rc;
    HRN_CHECK(ref && views && shifts, -2, "hrn_mncc_search: null argument");
    return hrn_launch_mncc_search(ref, ref_mask, views, view_masks, B, V, H, W, P, levels, radius, shifts, trace, (hipStream_t)stream);
}

int hrn_mncc_apply(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                   float* out_valid, void* stream) {
    if (int rc = mncc_check("hrn_mncc_apply", B, V, H, W)) return rc;
    HRN_CHECK(views && shifts && out && out_valid, -2, "hrn_mncc_apply: null argument");
    return hrn_launch_mncc_apply(views, view_masks, shifts, B, V, H, W, out, out_valid, (hipStream_t)stream);
}

// the same search and resampling for frames of any size, in tiles (registration_scene.hip)
static int mncc_scene_check(const char* who, int B, int V, int H, int W) {
    if (int rc = mncc_check(who, B, V, H, W, HRN_MNCC_SCENE_MIN_SIDE, HRN_MNCC_SCENE_MAX_SIDE)) return rc;
    MNCC_LIMIT(hrn_mncc_scene_grid_fits(B, V, H, W), "%s: bad batch B=%d V=%d: the tiles of %d x %d frames exceed one launch", who, B, V, H, W);
    return 0;
}

size_t hrn_mncc_scene_workspace_bytes(int B, int V, int H, int W, int P) {
    if (mncc_scene_check(nullptr, B, V, H, W) || mncc_check_points(nullptr, P)) return 0;
    return hrn_mncc_scene_workspace_bytes_impl(B, V, H, W, P);
}

int hrn_mncc_grid_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* centres, int B,
                        int V, int H, int W, int P, float width, float* scores, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = mncc_scene_check("hrn_mncc_grid_scene", B, V, H, W)) return rc;
    if (int rc = mncc_check_points("hrn_mncc_grid_scene", P)) return rc;
    HRN_CHECK(width > 0.f && width <= 8.f, -2, "hrn_mncc_grid_scene: width %g outside (0, 8]", (double)width);
    HRN_CHECK(ref && views && centres && scores && workspace, -2, "hrn_mncc_grid_scene: null argument");
    HRN_CHECK(workspace_bytes >= hrn_mncc_scene_workspace_bytes_impl(B, V, H, W, P), -3, "hrn_mncc_grid_scene: workspace too small");
    return hrn_launch_mncc_grid_scene(ref, ref_mask, views, view_masks, centres, B, V, H, W, P, width, scores, workspace, (hipStream_t)stream);
}

// hrn_mncc_search_scene (init null: from (0, 0)) and hrn_mncc_search_scene_from
static int mncc_search_scene(const char* who, const float* ref, const float* ref_mask, const float* views, const float* view_masks,
                             const float* init, int B, int V, int H, int W, int P, int levels, float radius, float* shifts, float* trace,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = mncc_scene_check(who, B, V, H, W)) return rc;
    if (int rc = mncc_check_search(who, P, levels, radius)) return rc;
    HRN_CHECK(ref && views && shifts && workspace, -2, "%s: null argument", who);
    HRN_CHECK(workspace_bytes >= hrn_mncc_scene_workspace_bytes_impl(B, V, H, W, P), -3, "%s: workspace too small", who);
    return hrn_launch_mncc_search_scene_from(ref, ref_mask, views, view_masks, init, B, V, H, W, P, levels, radius, shifts, trace, nullptr, 0,
                                             workspace, (hipStream_t)stream);
}

int hrn_mncc_search_scene(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                          int P, int levels, float radius, float* shifts, float* trace, void* workspace, size_t workspace_bytes,
                          void* stream) {
    return mncc_search_scene("hrn_mncc_search_scene", ref, ref_mask, views, view_masks, nullptr, B, V, H, W, P, levels, radius, shifts, trace,
                             workspace, workspace_bytes, stream);
}

int hrn_mncc_search_scene_from(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init, int B,
                               int V, int H, int W, int P, int levels, float radius, float* shifts, float* trace, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return mncc_search_scene("hrn_mncc_search_scene_from", ref, ref_mask, views, view_masks, init, B, V, H, W, P, levels, radius, shifts,
                             trace, workspace, workspace_bytes, stream);
}

int hrn_mncc_apply_scene(const float* views, const float* view_masks, const float* shifts, int B, int V, int H, int W, float* out,
                         float* out_valid, void* stream) {
    if (int rc = mncc_scene_check("hrn_mncc_apply_scene", B, V, H, W)) return rc;
    HRN_CHECK(views && shifts && out && out_valid, -2, "hrn_mncc_apply_scene: null argument");
    return hrn_launch_mncc_apply_scene(views, view_masks, shifts, B, V, H, W, out, out_valid, (hipStream_t)stream);
}

// the backward of hrn_mncc_apply_scene (resample_bwd.hip)
size_t hrn_mncc_apply_backward_workspace_bytes(int B, int V, int H, int W) {
    if (mncc_scene_check(nullptr, B, V, H, W)) return 0;
    return hrn_mncc_apply_backward_workspace_bytes_impl(B, V, H, W);
}

int hrn_mncc_apply_backward(const float* views, const float* shifts, const float* valid, const float* d_out, int B, int V, int H, int W,
                            float* d_views, float* d_shifts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = mncc_scene_check("hrn_mncc_apply_backward", B, V, H, W)) return rc;
    HRN_CHECK(d_views || d_shifts, -2, "hrn_mncc_apply_backward: d_views and d_shifts are both null: nothing to compute");
    HRN_CHECK(shifts && valid && d_out, -2, "hrn_mncc_apply_backward: null argument");
    if (d_shifts) {
        HRN_CHECK(views && workspace, -2, "hrn_mncc_apply_backward: d_shifts needs views and a workspace: null argument");
        HRN_CHECK(workspace_bytes >= hrn_mncc_apply_backward_workspace_bytes_impl(B, V, H, W), -3,
                  "hrn_mncc_apply_backward: workspace too small");
    }
    return hrn_launch_mncc_apply_backward(views, shifts, valid, d_out, B, V, H, W, d_views, d_shifts, workspace, (hipStream_t)stream);
}

// the sub-pixel searched cMSE / cPSNR loss (subpixel_loss.hip): the scene search's limits and the searched losses' border
static int subpixel_loss_check(const char* who, int B, int H, int W, int border, int metric) {
    if (int rc = mncc_scene_check(who, B, 1, H, W)) return rc;
    MNCC_LIMIT(border >= 0 && border <= 8, "%s: border %d outside 0..8", who, border);
    MNCC_LIMIT(2 * border < H && 2 * border < W, "%s: bad shape H=%d W=%d border=%d: the border must be below half of each side", who, H, W,
               border);
    MNCC_LIMIT(metric == 1 || metric == 2, "%s: metric must be 1 (cMSE) or 2 (cPSNR)", who);
    return 0;
}

size_t hrn_subpixel_loss_workspace_bytes(int B, int H, int W, int P) {
    if (mncc_scene_check(nullptr, B, 1, H, W) || mncc_check_points(nullptr, P)) return 0;
    const size_t fwd = hrn_subpixel_loss_forward_bytes_impl(B, H, W, P), bwd = hrn_subpixel_loss_backward_bytes_impl(B, H, W);
    return fwd > bwd ? fwd : bwd;
}

int hrn_subpixel_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int P, int levels,
                            float radius, int metric, float* out, double* stats, float* trace, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* who = "hrn_subpixel_loss_train";
    if (int rc = subpixel_loss_check(who, B, H, W, border, metric)) return rc;
    if (int rc = mncc_check_search(who, P, levels, radius)) return rc;
    HRN_CHECK(srs && hrs && maps && out && stats && workspace, -2, "%s: null argument", who);
    HRN_CHECK(workspace_bytes >= hrn_subpixel_loss_workspace_bytes(B, H, W, P), -3, "%s: workspace too small", who);
    return hrn_launch_subpixel_loss_train(srs, hrs, maps, B, H, W, border, P, levels, radius, metric, out, stats, trace, workspace,
                                          (hipStream_t)stream);
}

int hrn_subpixel_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B, int H,
                               int W, int border, int metric, float* d_srs, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "hrn_subpixel_loss_backward";
    if (int rc = subpixel_loss_check(who, B, H, W, border, metric)) return rc;
    HRN_CHECK(srs && hrs && maps && stats && d_out && d_srs && workspace, -2, "%s: null argument", who);
    HRN_CHECK(workspace_bytes >= hrn_subpixel_loss_backward_bytes_impl(B, H, W), -3, "%s: workspace too small", who);
    return hrn_launch_subpixel_loss_backward(srs, hrs, maps, stats, d_out, B, H, W, border, metric, d_srs, workspace, (hipStream_t)stream);
}

// a shift per block of tiles and the resampling by the field between them (registration_local.hip)
static int mncc_check_block(const char* who, int block) {
    MNCC_LIMIT(block >= HRN_MNCC_LOCAL_MIN_BLOCK && block <= HRN_MNCC_LOCAL_MAX_BLOCK && block % HRN_MNCC_SCENE_TILE == 0,
               "%s: bad block %d: a block must be a multiple of %d in %d..%d", who, block, HRN_MNCC_SCENE_TILE, HRN_MNCC_LOCAL_MIN_BLOCK,
               HRN_MNCC_LOCAL_MAX_BLOCK);
    return 0;
}

static int mncc_local_check(const char* who, int B, int V, int H, int W, int block) {
    if (int rc = mncc_scene_check(who, B, V, H, W)) return rc;
    if (int rc = mncc_check_block(who, block)) return rc;
    MNCC_LIMIT(hrn_mncc_local_grid_fits(B, V, H, W, block), "%s: bad batch B=%d V=%d: the blocks of %d x %d frames exceed one launch", who, B, V,
               H, W);
    return 0;
}

int hrn_mncc_local_blocks(int L, int block) {
    if (L < 1 || L > HRN_MNCC_SCENE_MAX_SIDE || mncc_check_block(nullptr, block)) return 0;
    return hrn_mncc_local_blocks_impl(L, block);
}

size_t hrn_mncc_local_workspace_bytes(int B, int V, int H, int W, int P, int block) {
    if (mncc_local_check(nullptr, B, V, H, W, block) || mncc_check_points(nullptr, P)) return 0;
    return hrn_mncc_local_workspace_bytes_impl(B, V, H, W, P, block);
}

int hrn_mncc_search_local(const float* ref, const float* ref_mask, const float* views, const float* view_masks, const float* init, int B, int V,
                          int H, int W, int P, int levels, float radius, int block, float min_valid, float* field, float* trace, float* ok,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = mncc_local_check("hrn_mncc_search_local", B, V, H, W, block)) return rc;
    if (int rc = mncc_check_search("hrn_mncc_search_local", P, levels, radius)) return rc;
    HRN_CHECK(min_valid >= 0.f && min_valid <= 1.f, -2, "hrn_mncc_search_local: min_valid %g outside [0, 1]", (double)min_valid);
    HRN_CHECK(ref && views && field && workspace, -2, "hrn_mncc_search_local: null argument");
    HRN_CHECK(workspace_bytes >= hrn_mncc_local_workspace_bytes_impl(B, V, H, W, P, block), -3, "hrn_mncc_search_local: workspace too small");
    return hrn_launch_mncc_search_local(ref, ref_mask, views, view_masks, init, B, V, H, W, P, levels, radius, block, min_valid, field, trace, ok,
                                        workspace, (hipStream_t)stream);
}

int hrn_mncc_apply_field(const float* views, const float* view_masks, const float* field, int B, int V, int H, int W, int block, float* out,
                         float* out_valid, void* stream) {
    if (int rc = mncc_local_check("hrn_mncc_apply_field", B, V, H, W, block)) return rc;
    HRN_CHECK(views && field && out && out_valid, -2, "hrn_mncc_apply_field: null argument");
    return hrn_launch_mncc_apply_field(views, view_masks, field, B, V, H, W, block, out, out_valid, (hipStream_t)stream);
}

// the masked pyramid and the coarse-to-fine search over it (registration_pyramid.hip)
int hrn_mncc_reduce2(const float* x, const float* mask, int N, int H, int W, float* out, float* out_mask, void* stream) {
    HRN_CHECK(N > 0, -2, "hrn_mncc_reduce2: bad plane count N=%d", N);
    HRN_CHECK(H >= HRN_MNCC_REDUCE_MIN_SIDE && H <= HRN_MNCC_SCENE_MAX_SIDE && W >= HRN_MNCC_REDUCE_MIN_SIDE && W <= HRN_MNCC_SCENE_MAX_SIDE, -2,
              "hrn_mncc_reduce2: bad shape H=%d W=%d: the sides of a plane must be %d..%d", H, W, HRN_MNCC_REDUCE_MIN_SIDE, HRN_MNCC_SCENE_MAX_SIDE);
    HRN_CHECK(hrn_mncc_reduce2_grid_fits((size_t)N, H, W), -2, "hrn_mncc_reduce2: N=%d planes of %d x %d exceed one launch", N, H, W);
    HRN_CHECK(x && out && out_mask, -2, "hrn_mncc_reduce2: null argument");
    return hrn_launch_mncc_reduce2(x, mask, (size_t)N, nullptr, nullptr, 0, H, W, out, out_mask, nullptr, nullptr, (hipStream_t)stream);
}

// every limit of hrn_mncc_search_pyramid.  Its size query has no levels and no radii and passes 1 for each: with radius 1 the reach
// rule cannot fire (2^HRN_MNCC_MAX_OCTAVES <= HRN_MNCC_PYRAMID_MAX_REACH).
static int mncc_pyramid_check(const char* who, int B, int V, int H, int W, int P, int octaves, int levels, float radius, int coarse_levels,
                              float refine_radius) {
    if (int rc = mncc_scene_check(who, B, V, H, W)) return rc;
    if (int rc = mncc_check_points(who, P)) return rc;
    if (int rc = mncc_check_levels(who, "levels", levels)) return rc;
    if (int rc = mncc_check_levels(who, "coarse_levels", coarse_levels)) return rc;
    MNCC_LIMIT(octaves >= 0 && octaves <= HRN_MNCC_MAX_OCTAVES, "%s: octaves %d outside 0..%d", who, octaves, HRN_MNCC_MAX_OCTAVES);
    if (int rc = mncc_check_radius(who, "radius", radius)) return rc;
    MNCC_LIMIT(radius * (float)(1 << octaves) <= HRN_MNCC_PYRAMID_MAX_REACH, "%s: radius %g over %d octaves reaches %g pixels, beyond %g", who,
               (double)radius, octaves, (double)radius * (1 << octaves), (double)HRN_MNCC_PYRAMID_MAX_REACH);
    MNCC_LIMIT(((H < W ? H : W) >> octaves) >= HRN_MNCC_SCENE_MIN_SIDE, "%s: bad shape H=%d W=%d: octave %d of the frame must be at least %d a side",
               who, H, W, octaves, HRN_MNCC_SCENE_MIN_SIDE);
    if (int rc = mncc_check_radius(who, "refine_radius", refine_radius)) return rc;
    MNCC_LIMIT(octaves == 0 || hrn_mncc_reduce2_grid_fits((size_t)B * V + (size_t)B, H, W),
               "%s: bad batch B=%d V=%d: the planes of %d x %d frames exceed one launch of the reduction", who, B, V, H, W);
    return 0;
}
static_assert((float)(1 << HRN_MNCC_MAX_OCTAVES) <= HRN_MNCC_PYRAMID_MAX_REACH, "the size query's radius 1 passes the reach rule");

size_t hrn_mncc_pyramid_workspace_bytes(int B, int V, int H, int W, int P, int octaves) {
    if (mncc_pyramid_check(nullptr, B, V, H, W, P, octaves, 1, 1.f, 1, 1.f)) return 0;
    return hrn_mncc_pyramid_workspace_bytes_impl(B, V, H, W, P, octaves);
}

int hrn_mncc_search_pyramid(const float* ref, const float* ref_mask, const float* views, const float* view_masks, int B, int V, int H, int W,
                            int P, int octaves, int levels, float radius, int coarse_levels, float refine_radius, float* shifts, float* trace,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "hrn_mncc_search_pyramid";
    if (int rc = mncc_pyramid_check(who, B, V, H, W, P, octaves, levels, radius, coarse_levels, refine_radius)) return rc;
    HRN_CHECK(ref && views && shifts && workspace, -2, "%s: null argument", who);
    HRN_CHECK(workspace_bytes >= hrn_mncc_pyramid_workspace_bytes_impl(B, V, H, W, P, octaves), -3, "%s: workspace too small", who);
    return hrn_launch_mncc_search_pyramid(ref, ref_mask, views, view_masks, B, V, H, W, P, octaves, levels, radius, coarse_levels, refine_radius,
                                          shifts, trace, workspace, (hipStream_t)stream);
}

}  // extern "C"
