// Input gradients of HRNet's training path: d lrs and d alphas (reference HRNet.py:198-204 and :113-132).  Both passes read
// tensors the backward already holds in its workspace and are memory-bound.  Deterministic: no atomics, fixed summation orders.
//
//   stem dgrad + median routing   the stem sees cat(lr_v, ref): d_in[c][q] = sum_co sum_tap W[co][c][tap] dA[q - tap][co]
//                                 (conv_transpose of the pre-activation gradient dA, 64 -> 2).  Channel 0 is d lrs[b, v]; channel 1,
//                                 summed over the V views of sample b in view order, is the gradient of the reference frame (the
//                                 lower median of lrs[b, :min(V, 9)]) and goes to ONE view per pixel: the lowest-indexed of the first
//                                 min(V, 9) views whose value equals the median.
//   alpha gradient                x_new = alice + a_bob * f at each fusion level: d a_bob = sum_{c, px} dsn * f, per-workgroup partials
//                                 and a fixed-order finish, like the weight-gradient finishes of backward.hip
#include "kernels.h"
#include "backward.h"

namespace {

// stem dgrad tile: 8 rows x 32 columns of pixels, one per thread, plus a 1-pixel halo; dA is staged through LDS 32 channels at a time
// (pixel stride 36 floats: ds_read_b128 of 16 consecutive pixels hits 16 distinct 4-bank groups)
constexpr int SD_TH = 8, SD_TW = 32, SD_HH = SD_TH + 2, SD_HW = SD_TW + 2, SD_CC = 32, SD_PS = SD_CC + 4;

// 4 consecutive elements of an activation tensor as loaded (f32: the four floats' bits; bf16: one pair; bf16x3: hi pair then lo pair),
// converted to f32 only when they are stored to LDS, so that the loads stay in flight across the computation
template <int ST> __device__ __forceinline__ u32x4 ld_raw(const void* p, size_t lo, size_t i4) {
    if constexpr (ST == HRN_BF16X3) {
        const u32x2 h = __builtin_nontemporal_load((const u32x2*)p + i4);
        const u32x2 l = __builtin_nontemporal_load((const u32x2*)((const unsigned char*)p + lo) + i4);
        return u32x4{h[0], h[1], l[0], l[1]};
    } else if constexpr (ST == HRN_BF16) {
        const u32x2 h = __builtin_nontemporal_load((const u32x2*)p + i4);
        return u32x4{h[0], h[1], 0u, 0u};
    } else {
        return __builtin_nontemporal_load((const u32x4*)p + i4);
    }
}
template <int ST> __device__ __forceinline__ f32x4 raw_to_f32(u32x4 r) {
    if constexpr (ST == HRN_BF16X3) {
        f32x4 o;
        o[0] = __uint_as_float(r[0] << 16) + __uint_as_float(r[2] << 16);
        o[1] = __uint_as_float(r[0] & 0xffff0000u) + __uint_as_float(r[2] & 0xffff0000u);
        o[2] = __uint_as_float(r[1] << 16) + __uint_as_float(r[3] << 16);
        o[3] = __uint_as_float(r[1] & 0xffff0000u) + __uint_as_float(r[3] & 0xffff0000u);
        return o;
    } else if constexpr (ST == HRN_BF16) {
        return f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16),
                     __uint_as_float(r[1] & 0xffff0000u)};
    } else {
        return f32x4{__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3])};
    }
}

// wt[tap][co][c] = w[co][c][tap]: the stem weights (64, 2, 3, 3) with the 128 values of one tap contiguous
__global__ __launch_bounds__(256) void stem_dgrad_weights_kernel(const float* __restrict__ w, float* __restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * 18) return;
    const int co = i / 18, c = (i / 9) & 1, tap = i % 9;
    wt[(tap * 64 + co) * 2 + c] = w[i];
}

template <int ST>
__global__ __launch_bounds__(256) void stem_dgrad_route_kernel(const void* __restrict__ dA, const float* __restrict__ wt,
                                                               const float* __restrict__ lrs, const float* __restrict__ ref,
                                                               float* __restrict__ d_lrs, int B, int V, int H, int W) {
    __shared__ __attribute__((aligned(16))) float tile[SD_HH * SD_HW * SD_PS];
    const int tid = threadIdx.x, tx = tid & (SD_TW - 1), ty = tid / SD_TW;
    const int tiles_x = (W + SD_TW - 1) / SD_TW, tiles_y = (H + SD_TH - 1) / SD_TH, tiles = tiles_x * tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int y0 = (t / tiles_x) * SD_TH, x0 = (t % tiles_x) * SD_TW;
    const int gy = y0 + ty, gx = x0 + tx;
    const bool inside = gy < H && gx < W;
    const size_t hw = (size_t)H * W, pix = (size_t)gy * W + gx;
    const size_t lo = (size_t)B * V * hw * 64 * 2;          // bf16x3: byte offset of dA's lo plane
    // the view that receives the reference frame's gradient at this pixel
    int sel = 0;
    if (inside) {
        const float r = ref[(size_t)b * hw + pix];
        const int n = V < 9 ? V : 9;
        sel = -1;
        for (int i = 0; i < n; ++i)
            if (sel < 0 && lrs[((size_t)b * V + i) * hw + pix] == r) sel = i;
        if (sel < 0) sel = 0;                               // (only a NaN median matches no view)
    }
    // the halo tile of one (view, 32-channel chunk) as raw 16-byte units, NLD per thread: chunk c + 1 is in flight while chunk c is
    // computed from LDS
    constexpr int NU = SD_HH * SD_HW * (SD_CC / 4), NLD = (NU + 255) / 256;
    u32x4 raw[NLD];
    unsigned ok = 0;                                        // bit u: unit u lies in the image (else it is stored as zero padding)
    auto fetch = [&](int c) {
        const size_t img = (size_t)b * V + (c >> 1);
        const int k = c & 1;
        ok = 0;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int hp = i / (SD_CC / 4), q = i - hp * (SD_CC / 4);
            const int hy = hp / SD_HW, hx = hp - hy * SD_HW;
            const int yy = y0 + hy - 1, xx = x0 + hx - 1;
            const bool in = i < NU && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            ok |= (unsigned)in << u;
            // unconditional load from a clamped address (no branch: the loads of all units stay in flight together)
            const int cy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), cx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            raw[u] = ld_raw<ST>(dA, lo, (img * hw + (size_t)cy * W + cx) * 16 + k * (SD_CC / 4) + q);
        }
    };
    float acc1 = 0.f, keep = 0.f, o0 = 0.f, o1 = 0.f;
    fetch(0);
#pragma unroll 1
    for (int c = 0; c < 2 * V; ++c) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int hp = i / (SD_CC / 4), q = i - hp * (SD_CC / 4);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (i < NU) *(f32x4*)&tile[hp * SD_PS + q * 4] = (ok >> u) & 1 ? raw_to_f32<ST>(raw[u]) : z;
        }
        __syncthreads();
        if (c + 1 < 2 * V) fetch(c + 1);
        const int k = c & 1;
        // one tap at a time (not unrolled): its 64 weights of the chunk are contiguous in wt and come in by scalar loads
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            // forward: out[p] += W[tap] in[p + (ky-1, kx-1)]  =>  d in[q] += W[tap] dA[q - (ky-1, kx-1)]
            const float* src = &tile[((ty + 2 - ky) * SD_HW + (tx + 2 - kx)) * SD_PS];
            const float* wk = wt + ((size_t)tap * 64 + k * SD_CC) * 2;
#pragma unroll
            for (int j = 0; j < SD_CC / 4; ++j) {
                const f32x4 d = *(const f32x4*)&src[j * 4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o0 = fmaf(wk[(j * 4 + e) * 2], d[e], o0);
                    o1 = fmaf(wk[(j * 4 + e) * 2 + 1], d[e], o1);
                }
            }
        }
        if (k == 1) {                                       // view c / 2 complete
            const int v = c >> 1;
            acc1 += o1;
            if (inside) {
                if (v == sel) keep = o0;
                else d_lrs[((size_t)b * V + v) * hw + pix] = o0;
            }
            o0 = o1 = 0.f;
        }
    }
    if (inside) d_lrs[((size_t)b * V + sel) * hw + pix] = keep + acc1;
}

// The same data gradient for a reference frame that came from outside (hrn_hrnet_backward_ref): there is no median to route to, so d_lrs (or
// null) gets channel 0 alone and d_ref (or null) [B][H][W] channel 1 summed over the sample's views in view order.  The text of the kernel
// above with the routing taken out, as a kernel of its own: the routed kernel keeps its device code, register allocation included
template <int ST>
__global__ __launch_bounds__(256) void stem_dgrad_ref_kernel(const void* __restrict__ dA, const float* __restrict__ wt,
                                                             float* __restrict__ d_lrs, float* __restrict__ d_ref, int B, int V, int H,
                                                             int W) {
    __shared__ __attribute__((aligned(16))) float tile[SD_HH * SD_HW * SD_PS];
    const int tid = threadIdx.x, tx = tid & (SD_TW - 1), ty = tid / SD_TW;
    const int tiles_x = (W + SD_TW - 1) / SD_TW, tiles_y = (H + SD_TH - 1) / SD_TH, tiles = tiles_x * tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int y0 = (t / tiles_x) * SD_TH, x0 = (t % tiles_x) * SD_TW;
    const int gy = y0 + ty, gx = x0 + tx;
    const bool inside = gy < H && gx < W;
    const size_t hw = (size_t)H * W, pix = (size_t)gy * W + gx;
    const size_t lo = (size_t)B * V * hw * 64 * 2;          // bf16x3: byte offset of dA's lo plane
    // the halo tile of one (view, 32-channel chunk) as raw 16-byte units, NLD per thread: chunk c + 1 is in flight while chunk c is
    // computed from LDS
    constexpr int NU = SD_HH * SD_HW * (SD_CC / 4), NLD = (NU + 255) / 256;
    u32x4 raw[NLD];
    unsigned ok = 0;                                        // bit u: unit u lies in the image (else it is stored as zero padding)
    auto fetch = [&](int c) {
        const size_t img = (size_t)b * V + (c >> 1);
        const int k = c & 1;
        ok = 0;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int hp = i / (SD_CC / 4), q = i - hp * (SD_CC / 4);
            const int hy = hp / SD_HW, hx = hp - hy * SD_HW;
            const int yy = y0 + hy - 1, xx = x0 + hx - 1;
            const bool in = i < NU && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            ok |= (unsigned)in << u;
            // unconditional load from a clamped address (no branch: the loads of all units stay in flight together)
            const int cy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), cx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            raw[u] = ld_raw<ST>(dA, lo, (img * hw + (size_t)cy * W + cx) * 16 + k * (SD_CC / 4) + q);
        }
    };
    float acc1 = 0.f, o0 = 0.f, o1 = 0.f;
    fetch(0);
#pragma unroll 1
    for (int c = 0; c < 2 * V; ++c) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * 256;
            const int hp = i / (SD_CC / 4), q = i - hp * (SD_CC / 4);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (i < NU) *(f32x4*)&tile[hp * SD_PS + q * 4] = (ok >> u) & 1 ? raw_to_f32<ST>(raw[u]) : z;
        }
        __syncthreads();
        if (c + 1 < 2 * V) fetch(c + 1);
        const int k = c & 1;
        // one tap at a time (not unrolled): its 64 weights of the chunk are contiguous in wt and come in by scalar loads
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - ky * 3;
            // forward: out[p] += W[tap] in[p + (ky-1, kx-1)]  =>  d in[q] += W[tap] dA[q - (ky-1, kx-1)]
            const float* src = &tile[((ty + 2 - ky) * SD_HW + (tx + 2 - kx)) * SD_PS];
            const float* wk = wt + ((size_t)tap * 64 + k * SD_CC) * 2;
#pragma unroll
            for (int j = 0; j < SD_CC / 4; ++j) {
                const f32x4 d = *(const f32x4*)&src[j * 4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o0 = fmaf(wk[(j * 4 + e) * 2], d[e], o0);
                    o1 = fmaf(wk[(j * 4 + e) * 2 + 1], d[e], o1);
                }
            }
        }
        if (k == 1) {                                       // view c / 2 complete
            const int v = c >> 1;
            acc1 += o1;
            if (inside && d_lrs) d_lrs[((size_t)b * V + v) * hw + pix] = o0;
            o0 = o1 = 0.f;
        }
    }
    if (inside && d_ref) d_ref[(size_t)b * hw + pix] = acc1;
}

// partial[img * P + part] = sum over part `part` of image img of dsn * f (fp32 per thread, double across the block, fixed tree)
template <int ST>
__global__ __launch_bounds__(256) void alpha_grad_partial_kernel(const void* __restrict__ dsn, const void* __restrict__ f, size_t img4,
                                                                 int nimg, int P, double* __restrict__ partial) {
    __shared__ double red[4];
    const int img = blockIdx.x / P, part = blockIdx.x - img * P;
    const size_t lo = (size_t)nimg * img4 * 8;
    const size_t per = (img4 + P - 1) / P, beg = (size_t)part * per, end = beg + per < img4 ? beg + per : img4;
    float s = 0.f;
    for (size_t e = beg + threadIdx.x; e < end; e += 256) {
        const size_t i4 = (size_t)img * img4 + e;
        const f32x4 a = act_ld4<ST>(dsn, lo, i4), c = act_ld4<ST>(f, lo, i4);
        s = fmaf(a[0], c[0], s); s = fmaf(a[1], c[1], s); s = fmaf(a[2], c[2], s); s = fmaf(a[3], c[3], s);
    }
    double d = s;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// d_alphas[b][pair_last - v] = sum of the P partials of image b * half + v, in order
__global__ __launch_bounds__(256) void alpha_grad_finish_kernel(const double* __restrict__ partial, int nimg, int P, int half, int pair_last,
                                                                int V, float* __restrict__ d_alphas) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img >= nimg) return;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += partial[(size_t)img * P + p];
    const int b = img / half, v = img - b * half;
    d_alphas[(size_t)b * V + (pair_last - v)] = (float)s;
}

int alpha_parts(int nimg) {
    const int p = (2048 + nimg - 1) / nimg;
    return p < 1 ? 1 : (p > 64 ? 64 : p);
}

}  // namespace

size_t hrn_alpha_grad_scratch_bytes(int nimg) { return (size_t)nimg * alpha_parts(nimg) * sizeof(double); }

int hrn_launch_stem_dgrad_route(int dt, const void* dA, const float* w, float* wt, const float* lrs, const float* ref, float* d_lrs, int B,
                                int V, int H, int W, hipStream_t s) {
    const long tiles = (long)((W + SD_TW - 1) / SD_TW) * ((H + SD_TH - 1) / SD_TH);
    HRN_CHECK(tiles * B < (1L << 31), -2, "stem dgrad: %d samples of %d x %d exceed the grid", B, H, W);
    const double px = (double)B * V * H * W;
    HrnProfScope prof("stem_dgrad_route", 2.0 * 18 * 64 * px, px * (64.0 * 4 + 4) + (double)B * H * W * 4 * ((V < 9 ? V : 9) + 1), s);
    hipLaunchKernelGGL(stem_dgrad_weights_kernel, dim3((64 * 18 + 255) / 256), dim3(256), 0, s, w, wt);
    HRN_LAUNCH_ST(dt, stem_dgrad_route_kernel, dim3((unsigned)(tiles * B)), dim3(256), 0, s, dA, (const float*)wt, lrs, ref, d_lrs, B, V, H, W);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_stem_dgrad_ref(int dt, const void* dA, const float* w, float* wt, float* d_lrs, float* d_ref, int B, int V, int H, int W,
                              hipStream_t s) {
    HRN_CHECK(d_lrs || d_ref, -2, "stem dgrad: neither d_lrs nor d_ref is wanted");
    const long tiles = (long)((W + SD_TW - 1) / SD_TW) * ((H + SD_TH - 1) / SD_TH);
    HRN_CHECK(tiles * B < (1L << 31), -2, "stem dgrad: %d samples of %d x %d exceed the grid", B, H, W);
    const double px = (double)B * V * H * W;
    HrnProfScope prof("stem_dgrad_ref", 2.0 * 18 * 64 * px, px * (64.0 * 4 + 4) + (double)B * H * W * 4, s);
    hipLaunchKernelGGL(stem_dgrad_weights_kernel, dim3((64 * 18 + 255) / 256), dim3(256), 0, s, w, wt);
    HRN_LAUNCH_ST(dt, stem_dgrad_ref_kernel, dim3((unsigned)(tiles * B)), dim3(256), 0, s, dA, (const float*)wt, d_lrs, d_ref, B, V, H, W);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_alpha_grad(int dt, const void* dsn, const void* f, int half, int pair_last, float* d_alphas, int B, int V, size_t hw,
                          void* scratch, size_t scratch_bytes, hipStream_t s) {
    const int nimg = B * half, P = alpha_parts(nimg);
    HRN_CHECK(hrn_alpha_grad_scratch_bytes(nimg) <= scratch_bytes, -2, "alpha grad: scratch too small for %d images", nimg);
    HrnProfScope prof("alpha_grad", 2.0 * nimg * hw * 64, 2.0 * nimg * hw * 64 * 4, s);
    double* partial = (double*)scratch;
    const size_t img4 = hw * 16;
    HRN_LAUNCH_ST(dt, alpha_grad_partial_kernel, dim3(nimg * P), dim3(256), 0, s, dsn, f, img4, nimg, P, partial);
    hipLaunchKernelGGL(alpha_grad_finish_kernel, dim3((nimg + 255) / 256), dim3(256), 0, s, (const double*)partial, nimg, P, half, pair_last, V, d_alphas);
    HRN_LAUNCH_CHECK();
    return 0;
}
