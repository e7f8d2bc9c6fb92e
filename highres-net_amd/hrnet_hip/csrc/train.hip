// Training path of HRNet (fp32; bf16x3: every activation / gradient tensor a pair of bf16 planes, three bf16 MFMAs per product - the
// convolutions, data gradients and weight gradients then run on conv3x3_v6x3.hip / wgrad_x3.hip; or bf16: every activation / gradient
// tensor one bf16 plane, one bf16 MFMA per product with fp32 accumulation - conv3x3_r64.hip / conv3x3_v6.hip and the one-plane instance of
// wgrad_x3.hip.  The elementwise passes are the same kernels templated on the storage): a forward that keeps what the backward needs,
// and the backward itself
// (`srs = fusion_model(lrs, alphas)` ... `loss.backward()`, src/train.py:172-190).
//
// Forward (HRNet.py:186-211) is the inference kernel sequence with every intermediate kept in the training workspace:
//   encoder   a0 = PReLU(stem);  h_l = PReLU(conv(a_l));  r_l = PReLU(conv(h_l));  a_{l+1} = a_l + r_l;  stack_0 = conv(a_nl)
//   level     z = cat(s_i, s_partner);  t1 = PReLU(convA(z));  u = PReLU(convB(t1));  t2 = z + u;  f = PReLU(convC(t2));
//             stack_{l+1}[i] = s_i + alpha_partner f   (i < n/2)
//   decoder   sr = conv1x1(PReLU(deconv(stack_T)))       (kernel_size == stride == S, the upscale factor: 2, 3 or 4)
// Backward walks it in reverse with three primitives per convolution: PReLU backward on the stored post-activation
// (+ slope gradient), the weight/bias gradient (backward.hip), and the data gradient, which is the forward convolution
// kernel run on the transposed, tap-flipped weights.  All gradients are accumulated (+=) into the caller's buffers.
#include "../../../include/hrnet_hip.h"
#include "kernels.h"
#include "backward.h"
#include "hrnet_layout.h"

using namespace hrn;

namespace {

constexpr int TMAX = 16;

struct TrainWs {
    int T;                                  // fusion levels
    int n_in[TMAX + 1];                     // views entering level l (n_in[T] = views left at the end)
    size_t ref, a[HRN_MAX_RES_LAYERS + 1], h[HRN_MAX_RES_LAYERS], r[HRN_MAX_RES_LAYERS];
    size_t stack[TMAX + 1], t1[TMAX], u[TMAX], t2[TMAX], f[TMAX];
    size_t g[5];                            // backward: five gradient buffers of one full activation each
    size_t xpre;                            // backward: a recomputed pre-activation (used only behind a PReLU whose slope is <= 0)
    size_t wt, wtp, zero_bias, scratch, scratch_bytes;
    size_t dec_f, dec_g;                    // bf16 / bf16x3: f32 copies of the fused state and of its gradient (the decoder's backward is the fp32 kernel)
    size_t total;
};

// a fusion level's pair gather of its view stack (h pairs, partner of view v is last - v, vs views per sample); h == 0: a plain activation
struct PairGather { int h, last, vs; };

int num_cus() { return hrn_device_cus(); }

TrainWs train_ws(int nl, int B, int V, int H, int W) {
    TrainWs w;
    memset(&w, 0, sizeof w);
    const size_t hw = (size_t)H * W;
    const size_t S = (size_t)B * V * hw * 64 * 4;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = hrn_align_up(off + bytes, ALIGN); return o; };
    w.ref = take((size_t)B * hw * 4);
    for (int l = 0; l <= nl; ++l) w.a[l] = take(S);
    for (int l = 0; l < nl; ++l) { w.h[l] = take(S); w.r[l] = take(S); }
    int n = V, T = 0;
    w.n_in[0] = V;
    w.stack[0] = take(S);
    while (n / 2 > 0 && T < TMAX) {
        const int half = n / 2;
        const size_t s128 = (size_t)B * half * hw * 128 * 4, s64 = (size_t)B * half * hw * 64 * 4;
        w.t1[T] = take(s128); w.u[T] = take(s128); w.t2[T] = take(s128); w.f[T] = take(s64);
        w.stack[T + 1] = take(s64);
        n = half;
        ++T;
        w.n_in[T] = n;
    }
    w.T = T;
    for (int i = 0; i < 5; ++i) w.g[i] = take(S);
    w.xpre = take(S);
    w.wt = take((size_t)128 * 128 * 9 * 4);
    w.wtp = take((size_t)128 * 128 * 9 * 4);
    w.zero_bias = take(128 * 4);
    // one scratch for every scale: the decoder's largest (S = 4) is below the convolutions' anyway, so the size is scale-free
    size_t sc = hrn_bwd_scratch_bytes(num_cus());
    const size_t sd = hrn_decoder_bwd_scratch_bytes(num_cus(), 4);
    if (sd > sc) sc = sd;
    w.scratch = take(sc);
    w.scratch_bytes = sc;
    w.dec_f = take((size_t)B * hw * 64 * 4);
    w.dec_g = take((size_t)B * hw * 64 * 4);
    w.total = off;
    return w;
}

int check_train(int nl, int B, int V, int H, int W) {
    HRN_CHECK(nl >= 0 && nl <= HRN_MAX_RES_LAYERS, -2, "num_layers %d out of range 0..%d", nl, HRN_MAX_RES_LAYERS);
    HRN_CHECK(B > 0 && V > 0 && H > 0 && W > 0, -2, "empty input B=%d V=%d H=%d W=%d", B, V, H, W);
    HRN_CHECK(V < (1 << TMAX), -2, "too many views (%d)", V);
    return 0;
}

// `packed` and the training workspace are carved at ALIGN-byte offsets, and every dtype's kernels read them with 16-byte vector and
// LDS-DMA loads: both base pointers must be ALIGN-aligned (every hipMalloc and caching-allocator block is).  Checked on the host, so a
// bad pointer is refused before any launch.
int check_aligned(const char* fn, int dt, const void* pk, const void* tws) {
    HRN_CHECK((uintptr_t)pk % ALIGN == 0 && (uintptr_t)tws % ALIGN == 0, -2,
              "%s: packed (%p) and train_ws (%p) must be %zu-byte aligned for the blob and workspace layout of dtype %d", fn, pk, tws,
              (size_t)ALIGN, dt);
    return 0;
}

// y = conv3x3(x) (+ PReLU) of site c on the forward kernel; x is the activation `in`, or with pg.h > 0 the pair gather of the view stack
// `in` (M / pg.h samples).  With `nonpos_slope` (the backward's recompute) y is the pre-activation, and the launch does nothing unless
// that slope, read on the device, is <= 0 (ConvParams::only_if_nonpos)
int conv_fwd(int dt, const void* pk, const ConvSite& c, const void* in, PairGather pg, void* y, int M, int H, int W, hipStream_t s,
             const float* nonpos_slope = nullptr) {
    const size_t hw = (size_t)H * W;
    ConvParams p = conv_base(M, H, W);
    if (pg.h > 0) {
        p.in_pair = 1; p.stack = in; p.pair_h = pg.h; p.pair_last = pg.last; p.pair_vs = pg.vs;
        p.stack_lo = hrn_lo_of(dt, (size_t)(M / pg.h) * pg.vs * hw * 64);
    } else {
        p.in = in; p.in_lo = hrn_lo_of(dt, (size_t)M * hw * c.cin);
    }
    p.out = y; p.out_lo = hrn_lo_of(dt, (size_t)M * hw * c.cout);
    conv_site(p, pk, c);
    if (nonpos_slope) { p.slope = nullptr; p.only_if_nonpos = nonpos_slope; }
    return hrn_launch_conv3x3(dt, c.cin, c.cout, p, s, false);
}

// z + u for the pair gather z of a level: t2[b*half + i][p][c] = (c < 64 ? s_i : s_partner)[p][c % 64] + u[...]
template <int ST>
__global__ __launch_bounds__(256) void pair_add_kernel(const void* __restrict__ stack, int n_in, int half, int pair_last,
                                                       const void* __restrict__ u, void* __restrict__ t2, size_t hw, int B) {
    const size_t total = (size_t)B * half * hw * 32;            // float4 units, 32 per pixel
    const size_t lo_s = (size_t)B * n_in * hw * 128, lo_u = total * 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pixg = i >> 5;
        const int part = (int)(i & 31);
        const size_t img = pixg / hw, pix = pixg - img * hw;
        const int b = (int)(img / half), v = (int)(img - (size_t)b * half);
        const int src = part < 16 ? v : pair_last - v;
        const f32x4 z = act_ld4<ST>(stack, lo_s, (((size_t)b * n_in + src) * hw + pix) * 16 + (part & 15));
        act_st4<ST>(t2, lo_u, i, z + act_ld4<ST>(u, lo_u, i));
    }
}

}  // namespace

int hrn_launch_pair_add(int dt, const void* stack, int n_in, int half, int pair_last, const void* u, void* t2, size_t hw, int B, hipStream_t s) {
    HRN_CHECK(stack && u && t2, -2, "pair_add: null argument");
    HRN_CHECK(B > 0 && half > 0 && hw > 0 && n_in >= 2 * half && pair_last >= half - 1 && pair_last < n_in, -2,
              "pair_add: bad level B=%d n_in=%d half=%d pair_last=%d hw=%zu", B, n_in, half, pair_last, hw);
    const size_t total4 = (size_t)B * half * hw * 32;
    size_t grid = (total4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    HRN_LAUNCH_ST(dt, pair_add_kernel, dim3((unsigned)grid), dim3(256), 0, s, stack, n_in, half, pair_last, u, t2, hw, B);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" {

size_t hrn_hrnet_train_workspace_bytes(int num_layers, int B, int V, int H, int W) {
    if (num_layers < 0 || num_layers > HRN_MAX_RES_LAYERS || B <= 0 || V <= 0 || H <= 0 || W <= 0 || V >= (1 << TMAX)) return 0;
    return train_ws(num_layers, B, V, H, W).total;
}

// The backward of every hrn_hrnet_backward* entry point (abi_fixed.hip holds the forms with an argument fixed).  A NULL field of `Gr` is
// a frozen parameter; with every field set, every gradient is produced.  A launch is left out only when nothing downstream reads
// any of its outputs; what runs computes what it computes on the full path, so every produced gradient is bit-identical to it.
//   need_ds[t]   the gradient of the views entering fusion level t (t = T: the decoder's data gradient, t = 0: d stack_0)
//   need_da[l]   the gradient of the encoder activation a_l (l = 0: the stem's output)
// Decoder parameters need only the decoder's weight-gradient part; fusion parameters (shared by every level) and d_alphas (alpha
// residual only) every level's data gradient above them; encoder / stem parameters and d_lrs the chain down to stack_0.
//   ext_ref      the reference frame of hrn_hrnet_forward_train_ref (null: the forward's own median, in the workspace); then d_lrs is the
//                stem's channel 0 alone and d_ref (or null) its channel 1 summed over the sample's views
static int backward_impl(const void* pk, int dt, int scale, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas,
                         const float* ext_ref, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, float* d_lrs,
                         float* d_alphas, float* d_ref, void* tws, size_t tws_bytes, void* stream) {
    int rc;
    HRN_CHECK(hrn_scale_ok(scale), -2, "hrn_hrnet_backward: scale must be 2, 3 or 4 (got %d)", scale);
    HRN_CHECK(dt == HRN_F32 || dt == HRN_BF16 || dt == HRN_BF16X3, -2, "hrn_hrnet_backward: dtype must be HRN_DTYPE_F32, HRN_DTYPE_BF16 or HRN_DTYPE_BF16X3 (got %d)", dt);
    HRN_CHECK(pk && Pr && Gr && lrs && alphas && d_sr && tws, -2, "hrn_hrnet_backward: null argument");
    if ((rc = check_aligned("hrn_hrnet_backward", dt, pk, tws))) return rc;
    const int nl = Pr->num_layers;
    if ((rc = check_train(nl, B, V, H, W))) return rc;
    const TrainWs L = train_ws(nl, B, V, H, W);
    HRN_CHECK(tws_bytes >= L.total, -3, "hrn_hrnet_backward: workspace too small (%zu < %zu)", tws_bytes, L.total);
    for (int t = 0; d_alphas && t < L.T; ++t)
        HRN_CHECK(hrn_alpha_grad_scratch_bytes(B * (L.n_in[t] / 2)) <= L.scratch_bytes, -3, "hrn_hrnet_backward_in: scratch too small for d_alphas");
    // ---- what is needed
    auto want = [](const float* g) { return g != nullptr; };
    auto want_site = [&](int k) { const SiteParams g = site_params(Gr, nl, k); return want(g.w) || want(g.b) || want(g.a); };
    const int kF = site_enc_final(nl), kA = site_fres(nl, 0), kB = site_fres(nl, 1), kC = site_fout(nl);
    const bool dec = want(Gr->dec_w) || want(Gr->dec_b) || want(Gr->dec_a) || want(Gr->fin_w) || want(Gr->fin_b);
    const bool wA = want_site(kA), wB = want_site(kB), wC = want_site(kC), fuse = wA || wB || wC;
    const bool alpha = d_alphas && alpha_residual;
    bool need_da[HRN_MAX_RES_LAYERS + 1], need_ds[TMAX + 1];
    need_da[0] = want_site(SITE_STEM) || d_lrs || d_ref;
    for (int l = 0; l < nl; ++l) need_da[l + 1] = need_da[l] || want_site(site_enc(l, 0)) || want_site(site_enc(l, 1));
    need_ds[0] = need_da[nl] || want_site(kF);
    for (int t = 0; t < L.T; ++t) need_ds[t + 1] = need_ds[t] || fuse || alpha;

    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)H * W;
    const int M = B * V, cus = num_cus();
    void* sc = at(tws, L.scratch);
    void* G[5];
    for (int i = 0; i < 5; ++i) G[i] = at(tws, L.g[i]);
    HRN_HIP(hipMemsetAsync(at(tws, L.zero_bias), 0, 128 * 4, s));
    // d alphas: views that are never bob (view 0, views dropped by parity) and every view without the alpha residual get 0
    if (d_alphas) HRN_HIP(hipMemsetAsync(d_alphas, 0, (size_t)B * V * 4, s));
    if (!dec && !need_ds[L.T]) return 0;
    // gradients are handed over as mutable buffers in a params-shaped struct
    auto mut = [](const float* p) { return const_cast<float*>(p); };
    const HrnetLayout P = hrnet_layout(dt, nl, scale);
    void* xpre = at(tws, L.xpre);
    // dx = conv3x3(g, W^T flipped) (+ res): the data gradient of site c's convolution, from its raw weights w [cout][cin][3][3]
    auto conv_dgrad = [&](const ConvSite& c, const float* w, const void* g, void* dx, const void* res, int Mi) -> int {
        return hrn_conv_dgrad(dt, c.cin, c.cout, w, g, dx, res, Mi, H, W, (float*)at(tws, L.wt), at(tws, L.wtp), (const float*)at(tws, L.zero_bias), s);
    };
    // The backward of y = PReLU(conv(x)) at site k, for Mi images; x is `in`, plain or with pg.h > 0 pair-gathered, as in conv_fwd.
    //   prelu   gx = d pre-activation from g = d y (may alias), + the slope and bias gradients where wanted.  It works from the stored
    //           post-activation y while the slope is positive; for a slope <= 0 (the reference allows any) the pre-activation is first
    //           recomputed into `xpre` - a launch gated on the device: no host round trip, ~3 us per PReLU in the usual case
    //   then the weight gradient where wanted, and with `dx` the data gradient dx = dgrad(gx) (+ res)
    auto site_bwd = [&](int k, const void* in, PairGather pg, const void* y, const void* g, void* gx, int Mi, bool prelu, void* dx,
                        const void* res) -> int {
        const ConvSite& c = P.site[k];
        const SiteParams p = site_params(Pr, nl, k), gr = site_params(Gr, nl, k);
        if (prelu) {
            if ((rc = conv_fwd(dt, pk, c, in, pg, xpre, Mi, H, W, s, p.a))) return rc;
            if ((rc = hrn_launch_prelu_bwd_bias(dt, g, y, xpre, p.a, gx, (size_t)Mi * hw, c.cout, mut(gr.a), mut(gr.b), sc, s))) return rc;
        }
        if (want(gr.w) && (rc = hrn_launch_conv_wgrad(dt, pg.h ? nullptr : in, pg.h ? in : nullptr, pg.h > 0, pg.h, pg.last, pg.vs, gx, Mi, H, W,
                                                      c.cin, c.cout, mut(gr.w), sc, cus, s)))
            return rc;
        return dx ? conv_dgrad(c, p.w, gx, dx, res, Mi) : 0;
    };

    // ---- decoder: d_sr -> d stack_T (one view left)                                  HRNet.py:147-156,167-169
    // (one launch gives the weight-gradient partials and d stack_T; its finish, which only sums the partials, runs for decoder parameters)
    void* dsn = G[0];                       // gradient of the views leaving the current level
    // the decoder's backward is the fp32 kernel (33 MB of state at the training shape): from planes, the fused state goes in as f32 and
    // its gradient comes back as planes
    const bool planes = dt != HRN_F32;
    const size_t nf = (size_t)B * L.n_in[L.T] * hw * 64;
    float* ff = (float*)at(tws, planes ? L.dec_f : L.stack[L.T]);
    float* fg = planes ? (float*)at(tws, L.dec_g) : (float*)dsn;
    if (planes && (rc = hrn_launch_planes_to_f32(at(tws, L.stack[L.T]), hrn_lo_of(dt, nf), ff, nf, s))) return rc;
    if ((rc = hrn_launch_decoder_bwd(ff, d_sr, Pr->dec_w, Pr->dec_b, Pr->dec_a, Pr->fin_w, fg, mut(Gr->dec_w), mut(Gr->dec_b), mut(Gr->dec_a),
                                     mut(Gr->fin_w), mut(Gr->fin_b), B, H, W, sc, cus, s, scale))) return rc;
    if (planes && need_ds[L.T] && (rc = hrn_launch_f32_to_planes(fg, dsn, hrn_lo_of(dt, nf), nf, s))) return rc;
    if (!need_ds[L.T]) return 0;

    // ---- fusion levels, last to first                                                HRNet.py:113-132
    // below: the level's input gradient ds is read (a lower level or the encoder); each convolution's PReLU backward runs when its data
    // gradient or one of its own parameters is wanted, and its data gradient when the PReLU backward before it runs
    for (int t = L.T - 1; t >= 0; --t) {
        const int n = L.n_in[t], half = n / 2, pair_last = n - (n & 1) - 1, Mh = B * half;
        const bool below = need_ds[t];
        const bool prA = below || wA, prB = prA || wB, dgC = prB || below, prC = dgC || wC;
        const void* st = at(tws, L.stack[t]);
        // every G buffer holds B*V*hw*64 floats; Mh <= B*V/2, so one buffer also holds an [Mh][hw][128] tensor
        void* y1 = G[1];                   // d t2               [Mh][hw][128]; dead before ds is written into the same buffer
        void* ds = G[1];                   // gradient of the views entering the level  [B*n][hw][64]
        void* x1 = G[2];                   // df / gC            [Mh][hw][64]
        void* y3 = G[3];                   // d t1 / gA          [Mh][hw][128]
        void* y2 = G[4];                   // gB, later dz       [Mh][hw][128]
        if (prC && (rc = hrn_launch_fuse_df(dt, dsn, alphas, V, pair_last, half, alpha_residual, x1, hw, B, s))) return rc;
        // x_new = alice + a_bob f: d a_bob = sum dsn f while both are live (the scratch is free until the PReLU backward below)
        if (alpha && (rc = hrn_launch_alpha_grad(dt, dsn, at(tws, L.f[t]), half, pair_last, d_alphas, B, V, hw, sc, L.scratch_bytes, s)))
            return rc;
        // f = PReLU(convC(t2))
        if ((rc = site_bwd(kC, at(tws, L.t2[t]), {}, at(tws, L.f[t]), x1, x1, Mh, prC, dgC ? y1 : nullptr, nullptr))) return rc;
        // t2 = z + u, u = PReLU(convB(t1))
        if ((rc = site_bwd(kB, at(tws, L.t1[t]), {}, at(tws, L.u[t]), y1, y2, Mh, prB, prA ? y3 : nullptr, nullptr))) return rc;
        // t1 = PReLU(convA(z));  dz = d t2 + dgradA(gA)
        if ((rc = site_bwd(kA, st, {half, pair_last, n}, at(tws, L.t1[t]), y3, y3, Mh, prA, below ? y2 : nullptr, y1))) return rc;
        if (!below) continue;               // (then no level below and not the encoder reads ds: the levels left run only their alpha_grad)
        // dz -> the two views of each pair (+ the alice pass-through)
        if ((rc = hrn_launch_fuse_scatter(dt, dsn, y2, n, half, pair_last, alpha_residual, ds, hw, B, s))) return rc;
        void* tmp = G[0]; G[0] = G[1]; G[1] = tmp;
        dsn = G[0];
    }
    if (!need_ds[0]) return 0;

    // ---- encoder                                                                     HRNet.py:51-60,62-74
    void* dA = G[1];
    const SiteParams gF = site_params(Gr, nl, kF);
    if (want(gF.w) && (rc = hrn_launch_conv_wgrad(dt, at(tws, L.a[nl]), nullptr, 0, 0, 0, 0, dsn, M, H, W, 64, 64, mut(gF.w), sc, cus, s))) return rc;
    if (want(gF.b) && (rc = hrn_launch_colsum(dt, dsn, (size_t)M * hw, 64, mut(gF.b), sc, s))) return rc;
    if (!need_da[nl]) return 0;
    if ((rc = conv_dgrad(P.site[kF], site_params(Pr, nl, kF).w, dsn, dA, nullptr, M))) return rc;
    void* e2 = G[2];
    void* e3 = G[3];
    for (int l = nl - 1; l >= 0; --l) {
        // a_{l+1} = a_l + r_l,  r_l = PReLU(conv2(h_l)),  h_l = PReLU(conv1(a_l));  d a_{l+1} (dA) is wanted here
        const int k1 = site_enc(l, 0), k2 = site_enc(l, 1);
        const bool pr1 = need_da[l] || want_site(k1), pr2 = pr1 || want_site(k2);
        if ((rc = site_bwd(k2, at(tws, L.h[l]), {}, at(tws, L.r[l]), dA, e2, M, pr2, pr1 ? e3 : nullptr, nullptr))) return rc;
        if ((rc = site_bwd(k1, at(tws, L.a[l]), {}, at(tws, L.h[l]), e3, e3, M, pr1, need_da[l] ? e2 : nullptr, dA))) return rc;
        if (!need_da[l]) return 0;
        void* tmp = dA; dA = e2; e2 = tmp;       // d a_l = d a_{l+1} + dgrad1(g1)
    }
    // stem: a_0 = PReLU(conv(cat(view, reference frame)))                               HRNet.py:200-204, :51-53
    const ConvSite& stem = P.site[SITE_STEM];
    const SiteParams pS = site_params(Pr, nl, SITE_STEM), gS = site_params(Gr, nl, SITE_STEM);
    const float* ref = ext_ref ? ext_ref : (const float*)at(tws, L.ref);
    if ((rc = hrn_launch_stem_pre(dt, lrs, hw, ref, V, hw, (const float*)at(pk, stem.w), (const float*)at(pk, stem.b), xpre, M, H, W,
                                  pS.a, s))) return rc;
    if ((rc = hrn_launch_prelu_bwd_bias(dt, dA, at(tws, L.a[0]), xpre, pS.a, dA, (size_t)M * hw, 64, mut(gS.a), mut(gS.b), sc, s))) return rc;
    if (want(gS.w) && (rc = hrn_launch_stem_wgrad(dt, lrs, hw, ref, V, hw, dA, M, H, W, mut(gS.w), sc, cus, s))) return rc;
    // d lrs: the stem's input gradient, channel 1 (the reference frame) routed to the view the median picked
    if (ext_ref) return d_lrs || d_ref ? hrn_launch_stem_dgrad_ref(dt, dA, pS.w, (float*)at(tws, L.wt), d_lrs, d_ref, B, V, H, W, s) : 0;
    if (d_lrs) return hrn_launch_stem_dgrad_route(dt, dA, pS.w, (float*)at(tws, L.wt), lrs, ref, d_lrs, B, V, H, W, s);
    return 0;
}

int hrn_hrnet_backward_sel(const void* pk, int dt, int scale, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas,
                           int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, float* d_lrs, float* d_alphas, void* tws,
                           size_t tws_bytes, void* stream) {
    return backward_impl(pk, dt, scale, Pr, alpha_residual, lrs, alphas, nullptr, B, V, H, W, d_sr, Gr, d_lrs, d_alphas, nullptr, tws, tws_bytes,
                         stream);
}

int hrn_hrnet_backward_ref(const void* pk, int dt, int scale, const hrn_hrnet_params* Pr, int alpha_residual, const float* lrs, const float* alphas,
                           const float* ref, int B, int V, int H, int W, const float* d_sr, const hrn_hrnet_params* Gr, float* d_lrs,
                           float* d_alphas, float* d_ref, void* tws, size_t tws_bytes, void* stream) {
    HRN_CHECK(ref, -2, "hrn_hrnet_backward_ref: null argument (ref)");
    return backward_impl(pk, dt, scale, Pr, alpha_residual, lrs, alphas, ref, B, V, H, W, d_sr, Gr, d_lrs, d_alphas, d_ref, tws, tws_bytes, stream);
}

// ext_ref: the reference frame (B,H,W) the stem reads in place of the median of lrs[:, :9] (null: the median, into the workspace)
static int forward_train_impl(const void* pk, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas,
                              const float* ext_ref, int B, int V, int H, int W, float* sr, void* tws, size_t tws_bytes, void* stream) {
    int rc;
    HRN_CHECK(hrn_scale_ok(scale), -2, "hrn_hrnet_forward_train: scale must be 2, 3 or 4 (got %d)", scale);
    if ((rc = check_train(nl, B, V, H, W))) return rc;
    HRN_CHECK(dt == HRN_F32 || dt == HRN_BF16 || dt == HRN_BF16X3, -2, "hrn_hrnet_forward_train: dtype must be HRN_DTYPE_F32, HRN_DTYPE_BF16 or HRN_DTYPE_BF16X3 (got %d)", dt);
    HRN_CHECK(pk && lrs && alphas && sr && tws, -2, "hrn_hrnet_forward_train: null argument");
    if ((rc = check_aligned("hrn_hrnet_forward_train", dt, pk, tws))) return rc;
    const TrainWs L = train_ws(nl, B, V, H, W);
    HRN_CHECK(tws_bytes >= L.total, -3, "hrn_hrnet_forward_train: workspace too small (%zu < %zu)", tws_bytes, L.total);
    const HrnetLayout P = hrnet_layout(dt, nl, scale);
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)H * W;
    const int M = B * V;
    // (an outside frame is read where it lies, by the stem here and by the backward, which is handed it again: no copy, no median launch)
    const float* ref = ext_ref ? ext_ref : (const float*)at(tws, L.ref);
    if (!ext_ref && (rc = hrn_launch_median(lrs, (float*)at(tws, L.ref), B, V, H, W, s))) return rc;
    const ConvSite& stem = P.site[SITE_STEM];
    if ((rc = hrn_launch_stem(dt, lrs, hw, ref, V, hw, nullptr, (const float*)at(pk, stem.w), (const float*)at(pk, stem.b),
                              (const float*)at(pk, stem.a), at(tws, L.a[0]), M, H, W, s, hrn_lo_of(dt, (size_t)M * hw * 64)))) return rc;
    for (int l = 0; l < nl; ++l) {
        if ((rc = conv_fwd(dt, pk, P.site[site_enc(l, 0)], at(tws, L.a[l]), {}, at(tws, L.h[l]), M, H, W, s))) return rc;
        if ((rc = conv_fwd(dt, pk, P.site[site_enc(l, 1)], at(tws, L.h[l]), {}, at(tws, L.r[l]), M, H, W, s))) return rc;
        if ((rc = hrn_launch_add(dt, at(tws, L.a[l]), at(tws, L.r[l]), at(tws, L.a[l + 1]), (size_t)M * hw * 64, s))) return rc;
    }
    if ((rc = conv_fwd(dt, pk, P.site[site_enc_final(nl)], at(tws, L.a[nl]), {}, at(tws, L.stack[0]), M, H, W, s))) return rc;
    for (int t = 0; t < L.T; ++t) {
        const int n = L.n_in[t], half = n / 2, pair_last = n - (n & 1) - 1;
        const void* st = at(tws, L.stack[t]);
        if ((rc = conv_fwd(dt, pk, P.site[site_fres(nl, 0)], st, {half, pair_last, n}, at(tws, L.t1[t]), B * half, H, W, s))) return rc;
        if ((rc = conv_fwd(dt, pk, P.site[site_fres(nl, 1)], at(tws, L.t1[t]), {}, at(tws, L.u[t]), B * half, H, W, s))) return rc;
        if ((rc = hrn_launch_pair_add(dt, st, n, half, pair_last, at(tws, L.u[t]), at(tws, L.t2[t]), hw, B, s))) return rc;
        if ((rc = conv_fwd(dt, pk, P.site[site_fout(nl)], at(tws, L.t2[t]), {}, at(tws, L.f[t]), B * half, H, W, s))) return rc;
        if ((rc = hrn_launch_fuse_update(dt, st, n, at(tws, L.f[t]), alphas, V, pair_last, half, alpha_residual,
                                         at(tws, L.stack[t + 1]), hw, B, s))) return rc;
    }
    // views left after the last level: 1 (or V itself for V == 1); torch.mean over them (HRNet.py:134) is the identity
    return hrn_launch_decoder(dt, at(tws, L.stack[L.T]), at(pk, P.dec_w), (const float*)at(pk, P.dec_b), (const float*)at(pk, P.dec_a),
                              (const float*)at(pk, P.fin_w), (const float*)at(pk, P.fin_b), sr, B, H, W, s,
                              hrn_lo_of(dt, (size_t)B * L.n_in[L.T] * hw * 64), scale);
}

int hrn_hrnet_forward_train_s(const void* pk, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas, int B, int V,
                              int H, int W, float* sr, void* tws, size_t tws_bytes, void* stream) {
    return forward_train_impl(pk, dt, nl, scale, alpha_residual, lrs, alphas, nullptr, B, V, H, W, sr, tws, tws_bytes, stream);
}

int hrn_hrnet_forward_train_ref(const void* pk, int dt, int nl, int scale, int alpha_residual, const float* lrs, const float* alphas,
                                const float* ref, int B, int V, int H, int W, float* sr, void* tws, size_t tws_bytes, void* stream) {
    HRN_CHECK(ref, -2, "hrn_hrnet_forward_train_ref: null argument (ref)");
    return forward_train_impl(pk, dt, nl, scale, alpha_residual, lrs, alphas, ref, B, V, H, W, sr, tws, tws_bytes, stream);
}

}  // extern "C"
