// The table of HRNet's 3x3 convolution sites and the packed-parameter layout (byte offsets into the blob hrn_hrnet_pack() fills),
// shared by api.hip and train.hip.  A site is one convolution with its bias and, but for the encoder's final one, its PReLU slope;
// sites are numbered in blob (= state-dict) order.  The decoder's tensors are no 3x3 site: they stay named fields and come last, so
// every offset before dec_w is the same for every upscale factor.
#pragma once
#include <string.h>
#include "../../../include/hrnet_hip.h"
#include "common.h"
#include "conv3x3.h"

namespace hrn {

constexpr size_t ALIGN = 256;

// site indices of a network with nl encoder residual blocks
constexpr int SITE_STEM = 0;                                          // 2 -> 64, raw f32 weights (stem.hip)
inline int site_enc(int l, int j) { return 1 + 2 * l + j; }           // conv j (0, 1) of encoder residual block l
inline int site_enc_final(int nl) { return 1 + 2 * nl; }              // no PReLU
inline int site_fres(int nl, int j) { return 2 + 2 * nl + j; }        // conv j of the fusion ResidualBlock, 128 -> 128
inline int site_fout(int nl) { return 4 + 2 * nl; }                   // the 128 -> 64 fusion conv
inline int num_sites(int nl) { return 5 + 2 * nl; }

struct ConvSite { int cin, cout; bool prelu; size_t w, b, a; };       // w, b, a: blob offsets (a: only with prelu)

struct HrnetLayout {
    ConvSite site[5 + 2 * HRN_MAX_RES_LAYERS];
    size_t dec_w, dec_b, dec_a, fin_w, fin_b;
    size_t total;
};

static inline HrnetLayout hrnet_layout(int dt, int nl, int scale) {
    HrnetLayout L;
    memset(&L, 0, sizeof L);
    const size_t es = hrn_esize(dt);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = hrn_align_up(off + bytes, ALIGN); return o; };
    for (int k = 0; k < num_sites(nl); ++k) {
        ConvSite& c = L.site[k];
        c.cin = k == SITE_STEM ? 2 : k >= site_fres(nl, 0) ? 128 : 64;
        c.cout = k == site_fres(nl, 0) || k == site_fres(nl, 1) ? 128 : 64;
        c.prelu = k != site_enc_final(nl);
        c.w = take(k == SITE_STEM ? 64 * 18 * 4 : (size_t)c.cin * c.cout * 9 * es);
        c.b = take(c.cout * 4);
        if (c.prelu) c.a = take(4);
    }
    // (Cin, Cout, S, S); bf16x3 keeps the fp32 decoder weights (es = 4)
    L.dec_w = take((size_t)64 * 64 * scale * scale * es); L.dec_b = take(64 * 4); L.dec_a = take(4);
    L.fin_w = take(64 * 4); L.fin_b = take(4);
    L.total = off;
    return L;
}

// (w, b, a) of site k in a params-shaped struct, parameters and gradients alike; NULL: the site has none (or, a gradient, is frozen)
struct SiteParams { const float *w, *b, *a; };
static inline SiteParams site_params(const hrn_hrnet_params* P, int nl, int k) {
    if (k == SITE_STEM) return {P->enc_init_w, P->enc_init_b, P->enc_init_a};
    if (k < site_enc_final(nl)) return {P->enc_res_w[k - 1], P->enc_res_b[k - 1], P->enc_res_a[k - 1]};
    if (k == site_enc_final(nl)) return {P->enc_final_w, P->enc_final_b, nullptr};
    const int j = k - site_fres(nl, 0);
    if (j < 2) return {P->fuse_res_w[j], P->fuse_res_b[j], P->fuse_res_a[j]};
    return {P->fuse_out_w, P->fuse_out_b, P->fuse_out_a};
}

static inline const unsigned char* at(const void* base, size_t off) { return (const unsigned char*)base + off; }
static inline unsigned char* at(void* base, size_t off) { return (unsigned char*)base + off; }

// the packed weights, bias and slope (NULL without PReLU) of site k as a convolution launch reads them
static inline void conv_site(ConvParams& p, const void* pk, const ConvSite& c) {
    p.wpk = at(pk, c.w); p.bias = (const float*)at(pk, c.b); p.slope = c.prelu ? (const float*)at(pk, c.a) : nullptr;
}

}  // namespace hrn
