// The shift-searched, brightness-corrected structural similarity cSSIM (the definition is in include/hrnet_hip.h):
// the score beside shift_loss.hip's cPSNR, over the same crops and the same (2 beta + 1)^2 offsets.  With s the centre crop of sr and,
// for the offset k = u (2 beta + 1) + v, g / m the crops of hr / map at (u, v) and b = bias_k, the compared pair is X = m g and
// Y = m (s + b); G is a separable T-tap window over "valid" positions.  Variances do not change when a constant leaves both images, and
// fp32 needs it to: on a bright, clear, low-contrast frame G X^2 - (G X)^2 is the difference of two numbers of the size of level^2.  So
// a tile takes c = the mean of g over the clear pixels of its hr window and filters the centred pair
//   X~ = m (g - c),   Y~ = m (s + b - c)          (X = X~ + c m, Y = Y~ + c m; m X~ = X~)
// and with p = G m, w = 1 - p:
//   mu_x = G X~ + c p,   v_x / cov_norm = (G X~^2 - (G X~)^2) + 2 c w G X~ + c^2 p w,       mu_y, v_y alike with Y~,
//   v_xy / cov_norm = (G X~Y~ - G X~ G Y~) + c w (G X~ + G Y~) + c^2 p w.
// w is filtered as G(1 - m) - (S - 1), S = the squared sum of the definition's taps: in a clear window G(1 - m) is exactly 0 and nothing
// of the size of c^2 is ever subtracted.  Only G Y~, G Y~^2, G X~Y~ depend on the offset (the bias enters as s - (c - b), one
// subtraction per pixel read); w, G X~ and v_x are functions of the hr position alone.
//
//   cssim_pre_kernel / cssim_pre_finish_kernel   n_k and bias_k of every sample and offset: fp64 sums of a run of crop pixels per
//                                                wave, the waves' sums added in index order
//   cssim_tile_kernel<T, BETA>                   a workgroup owns 16 x (64 - T + 1) pixels of one sample's SSIM map.  It stages the
//                                                (16 + T - 1) x 64 window of s, and of hr / map that window plus 2 beta rows and
//                                                columns, in LDS once (hr as X~); filters w, G X~, v_x over the tile plus 2 beta once;
//                                                then walks the offsets out of LDS.  Per offset, pass 1 runs down the columns: a
//                                                lane owns a window column (64 lanes = the 64 columns, a wave per 4 map rows),
//                                                reads 4 + T - 1 rows of s / X~ / m once each and slides the taps over them in
//                                                registers.  Pass 2 runs along the rows: a lane owns 4 map pixels of one row, reads
//                                                4 + T - 1 values per field once and slides again; the rows' stride of 65 and the
//                                                lanes' 4-float spacing put a wave's 64 reads on 64 banks.  The SSIM of its 4 pixels is
//                                                fp32; their sum, and everything above it, fp64 (wave_sums.h).
//   cssim_finish_kernel                          adds the tiles' (and their waves') sums in index order, divides by the map's size,
//                                                writes `scores` and takes the lowest k of maximal score among n_k > 0.
// No atomics, nothing returns to the host; the sums' order depends on the frame's shape alone, so a sample's result does not depend on
// the batch around it and two runs give the same bits.
#include "kernels.h"
#include "wave_sums.h"
#include <math.h>

#pragma clang fp contract(off)      // every fused multiply-add is written out: `scores` must not depend on what the compiler fuses

namespace {

constexpr int CS_MAX_BORDER = 8;
constexpr int CS_MAX_TAPS = 11;
constexpr int CS_WIN = 64;          // window columns of a tile: one lane per column in pass 1
constexpr int CS_TH = 16;           // map rows of a tile: 4 waves x CS_RUN
constexpr int CS_RUN = 4;           // map rows per lane in pass 1, map pixels per lane in pass 2
constexpr int CS_VS = CS_WIN + 1;   // row stride of the pass-1 output: odd, so that lanes on different rows hit different banks
constexpr int CS_PRE_PIX = 8;       // crop pixels per thread of the pre-pass
constexpr int CS_PRE_RUN = 256 * CS_PRE_PIX;

struct Taps { float w[CS_MAX_TAPS]; };

__host__ __device__ constexpr int cs_tw(int T) { return CS_WIN - T + 1; }                 // map columns of a tile
__host__ __device__ constexpr int cs_acs(int T, int beta) {                                   // row stride of the hr-position fields: 1 mod 4
    const int ac = cs_tw(T) + 2 * beta;
    return ac + ((1 - ac) & 3);
}

// the LDS of a tile, in floats: S | G (X~) | A (3 fields) | V | M (bytes)
struct TileLds { int s, g, a, v, m, total; };
__host__ __device__ constexpr TileLds cs_lds(int T, int beta) {
    const int wr = CS_TH + T - 1, gr = wr + 2 * beta, gc = CS_WIN + 2 * beta, ar = CS_TH + 2 * beta;
    TileLds l = {0, 0, 0, 0, 0, 0};
    l.s = 0;
    l.g = l.s + wr * CS_WIN;
    l.a = l.g + gr * gc;
    l.v = l.a + 3 * ar * cs_acs(T, beta);
    l.m = l.v + 3 * CS_TH * CS_VS + 16;     // pass 2's lanes past the tile's last column read up to 9 floats past a row's end: the pad
    l.total = l.m + (gr * gc + 3) / 4;
    return l;
}

// grid (runs, B).  A thread owns CS_PRE_PIX pixels of the flattened crop; pre [B][runs][nk][4 waves][2] = {sum m, sum m (g - s)}.
__global__ __launch_bounds__(256) void cssim_pre_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                        const float* __restrict__ maps, int H, int W, int border, int clip,
                                                        double* __restrict__ pre) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = 2 * border + 1, nk = nb * nb;
    const int h = H - 2 * border, w = W - 2 * border;
    const size_t npix = (size_t)h * w, img = (size_t)blockIdx.y * H * W;
    const float* sr = srs + img;
    const float* hr = hrs + img;
    const float* mp = maps + img;
    float s[CS_PRE_PIX];
    int at[CS_PRE_PIX];             // the pixel's index in hr at offset (0, 0); H W < 2^31 is checked by the caller
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < CS_PRE_PIX; ++j) {
        const size_t p = (size_t)blockIdx.x * CS_PRE_RUN + tid + 256 * j;
        const bool in = p < npix;
        const int y = in ? (int)(p / w) : 0, x = in ? (int)(p - (size_t)y * w) : 0;
        at[j] = y * W + x;
        float t = in ? sr[(size_t)(y + border) * W + (x + border)] : 0.f;
        if (clip) t = t != t ? t : fminf(fmaxf(t, 0.f), 1.f);           // torch.clamp keeps NaN
        s[j] = t;
        valid |= (unsigned)in << j;
    }
    double* out = pre + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * nk) * 8 + wave * 2;
    for (int k = 0; k < nk; ++k) {
        const int u = k / nb, v = k - u * nb, off = u * W + v;
        double a[2] = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < CS_PRE_PIX; ++j) {
            if (!((valid >> j) & 1)) continue;
            const double mm = mp[at[j] + off] != 0.f ? 1.0 : 0.0;
            const double d = (double)hr[at[j] + off] - (double)s[j];
            a[0] += mm;
            a[1] += mm * d;
        }
        WaveSums<2, 0>::run(a, lane);
        if (lane < 2) out[(size_t)k * 8 + wave_sums_index<2>(lane)] = a[0];
    }
}

// grid (B).  nbias [B][nk][2] = {n_k, bias_k}: the runs and their waves in index order.
__global__ __launch_bounds__(256) void cssim_pre_finish_kernel(const double* __restrict__ pre, int runs, int nk, int correct_bias,
                                                               double* __restrict__ nbias) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < nk; k += 256) {
        double s0 = 0.0, s1 = 0.0;
        for (int r = 0; r < runs; ++r) {
            const double* p = pre + (((size_t)b * runs + r) * nk + k) * 8;
#pragma unroll
            for (int q = 0; q < 4; ++q) { s0 += p[2 * q]; s1 += p[2 * q + 1]; }
        }
        nbias[((size_t)b * nk + k) * 2] = s0;
        nbias[((size_t)b * nk + k) * 2 + 1] = correct_bias && s0 > 0.0 ? s1 / s0 : 0.0;
    }
}

// the T taps down (DOWN) or along (!DOWN) `src`: dst[r * dstride + c] = sum_o w[o] src(r + o, c) or src(r, c + o), r < rows, c < cols
template <int T, bool DOWN, class Src>
__device__ __forceinline__ void cs_filter(const Taps& tp, Src src, float* dst, int dstride, int rows, int cols, int tid) {
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        float a = tp.w[0] * src(r, c);
#pragma unroll
        for (int o = 1; o < T; ++o) a = fmaf(tp.w[o], DOWN ? src(r + o, c) : src(r, c + o), a);
        dst[r * dstride + c] = a;
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
// two fields share a tap: one packed multiply-add (v_pk_fma_f32), each half rounded as fmaf rounds it
__device__ __forceinline__ f32x2 fma2(float w, f32x2 p, f32x2 a) { return __builtin_elementwise_fma(f32x2{w, w}, p, a); }

// grid (tiles, B), dynamic LDS cs_lds(T, BETA).total floats.  partial [B][tiles][nk][4 waves] = the sum of the wave's SSIM values.
// The border is a template argument so that every LDS row stride is a constant and the rows' offsets fold into the instructions.
template <int T, int BETA>
__global__ __launch_bounds__(256) void cssim_tile_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                         const float* __restrict__ maps, const double* __restrict__ nbias, int H, int W,
                                                         int clip, int ntx, Taps tp, float cov_norm, float c1, float c2,
                                                         float tap_excess, double* __restrict__ partial) {
    constexpr int TW = cs_tw(T), WR = CS_TH + T - 1, NIN = CS_RUN + T - 1, border = BETA;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr TileLds L = cs_lds(T, BETA);
    static_assert(L.total * sizeof(float) <= 65536, "a tile's LDS fits what a launch gets without opting in");
    float* S = lds + L.s;
    float* G = lds + L.g;
    float* A = lds + L.a;
    float* V = lds + L.v;
    unsigned char* M = reinterpret_cast<unsigned char*>(lds + L.m);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nb = 2 * border + 1, nk = nb * nb;
    const int h = H - 2 * border, w = W - 2 * border, mh = h - T + 1, mw = w - T + 1;
    constexpr int GR = WR + 2 * border, GC = CS_WIN + 2 * border, AR = CS_TH + 2 * border, AC = TW + 2 * border, ACS = cs_acs(T, border);
    const int tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * CS_TH, x0 = tx * TW;            // the tile's origin: map == crop coordinates == hr coordinates at offset (0, 0)
    const size_t img = (size_t)blockIdx.y * H * W;
    const float* sr = srs + img;
    const float* hr = hrs + img;
    const float* mp = maps + img;

    // ---- stage the windows; what lies outside the crop / the frame is 0 and feeds only map pixels that are not counted
    for (int i = tid; i < WR * CS_WIN; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int y = y0 + r, x = x0 + c;
        float t = y < h && x < w ? sr[(size_t)(y + border) * W + (x + border)] : 0.f;
        if (clip) t = t != t ? t : fminf(fmaxf(t, 0.f), 1.f);
        S[i] = t;
    }
    for (int i = tid; i < GR * GC; i += 256) {
        const int r = i / GC, c = i - r * GC;
        const int y = y0 + r, x = x0 + c;
        const bool in = y < H && x < W;
        const size_t j = (size_t)y * W + x;
        G[i] = in ? hr[j] : 0.f;
        M[i] = in && mp[j] != 0.f;
    }
    __syncthreads();

    // ---- the tile's centre c: the mean of g over the clear pixels of its hr window (0 without one, or where it is not finite).  Every
    // thread sums its own pixels in index order, a wave's butterfly leaves one sum in all its lanes, and every thread adds the four
    // waves' sums in wave order: the same bits in every thread, and a function of the sample's own data and the tile's place alone.
    float cen;
    {
        float n = 0.f, sg = 0.f;
        for (int i = tid; i < GR * GC; i += 256) {
            const float m = (float)M[i];
            n += m;
            sg = fmaf(m, G[i], sg);
        }
#pragma unroll
        for (int mask = 1; mask < 64; mask <<= 1) { n += __shfl_xor(n, mask); sg += __shfl_xor(sg, mask); }
        if (lane == 0) { V[2 * wave] = n; V[2 * wave + 1] = sg; }
        __syncthreads();
        n = (V[0] + V[2]) + (V[4] + V[6]);
        sg = (V[1] + V[3]) + (V[5] + V[7]);
        cen = n > 0.f ? sg / n : 0.f;
        if (!(fabsf(cen) <= 3.0e38f)) cen = 0.f;
        __syncthreads();                                            // V is the filters' scratch next
    }
    for (int i = tid; i < GR * GC; i += 256) G[i] = (float)M[i] * (G[i] - cen);          // X~; a thread rewrites what it alone reads here
    __syncthreads();

    // ---- the fields of the hr position alone, over the tile plus 2 beta: A[f] = G(1 - m), G X~, G X~^2 ...
    for (int f = 0; f < 3; ++f) {
        auto field = [&](int r, int c) {
            const int i = r * GC + c;
            const float x = G[i];
            return f == 0 ? 1.f - (float)M[i] : (f == 1 ? x : x * x);
        };
        cs_filter<T, true>(tp, field, V, GC, AR, GC, tid);
        __syncthreads();
        cs_filter<T, false>(tp, [&](int r, int c) { return V[r * GC + c]; }, A + f * AR * ACS, ACS, AR, AC, tid);
        __syncthreads();
    }
    // ... made w, G X~, v_x.  A thread reads back the elements it wrote itself; pass 2 reads them behind the offset loop's first barrier.
    for (int i = tid; i < AR * AC; i += 256) {
        const int r = i / AC, a = r * ACS + (i - r * AC);
        const float w = A[a] - tap_excess, ax = A[AR * ACS + a], axx = A[2 * AR * ACS + a];
        const float cw = cen * w, e = (cen * (1.f - w)) * cw;
        A[a] = w;
        A[2 * AR * ACS + a] = cov_norm * (fmaf(2.f * cw, ax, fmaf(-ax, ax, axx)) + e);
    }

    // pass 1: window column `lane`, map rows 4 wave ..; pass 2: map row 4 wave + lane / 16, map columns 4 (lane % 16) ..
    const int py = CS_RUN * wave + (lane >> 4), px = CS_RUN * (lane & 15);
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < CS_RUN; ++j) valid |= (unsigned)(px + j < TW && y0 + py < mh && x0 + px + j < mw) << j;
    const double* nbk = nbias + (size_t)blockIdx.y * nk * 2;
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + tile) * nk * 4 + wave;

    for (int k = 0; k < nk; ++k) {
        const int u = k / nb, v = k - u * nb;
        {
            f32x2 p01[NIN];                                         // (Y~, Y~^2)
            float p2[NIN];                                          // X~ Y~
            const float cs = (float)((double)cen - nbk[2 * k + 1]); // Y~ = m (s - (c - b))
            const int r0 = CS_RUN * wave;
            const float* Sp = S + r0 * CS_WIN + lane;
            const int g0 = (r0 + u) * GC + lane + v;
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const float t = Sp[i * CS_WIN] - cs, m = (float)M[g0 + i * GC], x = G[g0 + i * GC];
                const float mt = m * t;
                p01[i] = f32x2{mt, mt * t};
                p2[i] = x * t;
            }
            float* Vp = V + r0 * CS_VS + lane;
#pragma unroll
            for (int j = 0; j < CS_RUN; ++j) {
                f32x2 a01 = tp.w[0] * p01[j];
                float a2 = tp.w[0] * p2[j];
#pragma unroll
                for (int o = 1; o < T; ++o) {
                    a01 = fma2(tp.w[o], p01[j + o], a01);
                    a2 = fmaf(tp.w[o], p2[j + o], a2);
                }
                Vp[j * CS_VS] = a01.x;
                Vp[(CS_TH + j) * CS_VS] = a01.y;
                Vp[(2 * CS_TH + j) * CS_VS] = a2;
            }
        }
        __syncthreads();
        double sum = 0.0;
        {
            f32x2 q01[NIN];
            float q2[NIN];
            const float* Vq = V + py * CS_VS + px;
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                q01[i] = f32x2{Vq[i], Vq[CS_TH * CS_VS + i]};
                q2[i] = Vq[2 * CS_TH * CS_VS + i];
            }
            const int ai = (py + u) * ACS + px + v;
#pragma unroll
            for (int j = 0; j < CS_RUN; ++j) {
                f32x2 f01 = tp.w[0] * q01[j];
                float axy = tp.w[0] * q2[j];
#pragma unroll
                for (int o = 1; o < T; ++o) {
                    f01 = fma2(tp.w[o], q01[j + o], f01);
                    axy = fmaf(tp.w[o], q2[j + o], axy);
                }
                const float ay = f01.x, ayy = f01.y;
                const bool ok = (valid >> j) & 1;
                const int a = ok ? ai + j : 0;                      // the lanes past the tile's last column read nothing out of bounds
                const float w = A[a], ax = A[AR * ACS + a], vx = A[2 * AR * ACS + a];
                const float cp = cen * (1.f - w), cw = cen * w, e = cp * cw;
                const float mux = ax + cp, muy = ay + cp;
                const float vy = cov_norm * (fmaf(2.f * cw, ay, fmaf(-ay, ay, ayy)) + e);
                const float vxy = cov_norm * (fmaf(cw, ax + ay, fmaf(-ax, ay, axy)) + e);
                const float num = (2.f * mux * muy + c1) * (2.f * vxy + c2);
                const float den = (mux * mux + muy * muy + c1) * (vx + vy + c2);
                if (ok) sum += (double)(num / den);
            }
        }
        WaveSums<1, 0>::run(&sum, lane);
        if (lane == 0) out[(size_t)k * 4] = sum;
        __syncthreads();                                            // pass 2's readers of V are done
    }
}

// grid (B).  The tiles and their waves in index order; the lowest k of maximal score among n_k > 0 (strict >: a NaN is never selected).
__global__ __launch_bounds__(256) void cssim_finish_kernel(const double* __restrict__ partial, const double* __restrict__ nbias, int ntiles,
                                                           int nk, double inv_count, float* __restrict__ out, double* __restrict__ stats,
                                                           double* __restrict__ scores) {
    constexpr int MAXK = (2 * CS_MAX_BORDER + 1) * (2 * CS_MAX_BORDER + 1);
    __shared__ double sc[MAXK];
    const int b = blockIdx.x;
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    const double* nbk = nbias + (size_t)b * nk * 2;
    for (int k = threadIdx.x; k < nk; k += 256) {
        double sum = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            const double* p = partial + (((size_t)b * ntiles + t) * nk + k) * 4;
            sum += p[0]; sum += p[1]; sum += p[2]; sum += p[3];
        }
        const double v = nbk[2 * k] > 0.0 ? sum * inv_count : ninf;
        sc[k] = v;
        if (scores) scores[(size_t)b * nk + k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best = -1;
    double bv = ninf;
    for (int k = 0; k < nk; ++k)
        if (nbk[2 * k] > 0.0 && sc[k] > bv) { best = k; bv = sc[k]; }
    double* st = stats + 4 * (size_t)b;
    if (best < 0) {
        st[0] = 0.0; st[1] = 0.0; st[2] = __longlong_as_double(0x7ff8000000000000LL); st[3] = -1.0;
        out[b] = __int_as_float(0x7fc00000);
        return;
    }
    st[0] = nbk[2 * best]; st[1] = nbk[2 * best + 1]; st[2] = bv; st[3] = (double)best;
    out[b] = (float)bv;
}

struct Plan { int T, ntx; size_t tiles, runs, nk, pre, nbias, total; };
Plan plan_of(int B, int H, int W, int border, int window) {
    Plan p;
    p.T = window == 1 ? 7 : 11;
    const int mh = H - 2 * border - p.T + 1, mw = W - 2 * border - p.T + 1;
    p.ntx = (mw + cs_tw(p.T) - 1) / cs_tw(p.T);
    p.tiles = (size_t)p.ntx * ((mh + CS_TH - 1) / CS_TH);
    p.runs = ((size_t)(H - 2 * border) * (W - 2 * border) + CS_PRE_RUN - 1) / CS_PRE_RUN;
    p.nk = (size_t)(2 * border + 1) * (2 * border + 1);
    p.pre = 0;
    p.nbias = p.pre + (size_t)B * p.runs * p.nk * 8 * sizeof(double);
    const size_t part = p.nbias + (size_t)B * p.nk * 2 * sizeof(double);
    p.total = part + (size_t)B * p.tiles * p.nk * 4 * sizeof(double);
    return p;
}

template <int T, int BETA>
int launch_tile_at(const float* srs, const float* hrs, const float* maps, const double* nbias, int B, int H, int W, int clip, const Plan& p,
                   const Taps& tp, float cov_norm, float c1, float c2, float tap_excess, double* partial, hipStream_t stream) {
    constexpr int bytes = cs_lds(T, BETA).total * (int)sizeof(float);
    hipLaunchKernelGGL((cssim_tile_kernel<T, BETA>), dim3((unsigned)p.tiles, B), dim3(256), bytes, stream, srs, hrs, maps, nbias, H, W, clip,
                       p.ntx, tp, cov_norm, c1, c2, tap_excess, partial);
    HRN_LAUNCH_CHECK();
    return 0;
}

template <int T>
int launch_tile(const float* srs, const float* hrs, const float* maps, const double* nbias, int B, int H, int W, int border, int clip,
                const Plan& p, const Taps& tp, float cov_norm, float c1, float c2, float tap_excess, double* partial, hipStream_t stream) {
#define CS_AT(BETA) \
    case BETA: return launch_tile_at<T, BETA>(srs, hrs, maps, nbias, B, H, W, clip, p, tp, cov_norm, c1, c2, tap_excess, partial, stream)
    switch (border) {
        CS_AT(0); CS_AT(1); CS_AT(2); CS_AT(3); CS_AT(4); CS_AT(5); CS_AT(6); CS_AT(7);
        default: return launch_tile_at<T, 8>(srs, hrs, maps, nbias, B, H, W, clip, p, tp, cov_norm, c1, c2, tap_excess, partial, stream);
    }
#undef CS_AT
}

}  // namespace

size_t hrn_shift_cssim_workspace_bytes_impl(int B, int H, int W, int border, int window) { return plan_of(B, H, W, border, window).total; }

int hrn_launch_shift_cssim(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int window, int clip,
                           int correct_bias, float data_range, float* out, double* stats, double* scores, void* workspace,
                           hipStream_t stream) {
    const Plan p = plan_of(B, H, W, border, window);
    HRN_CHECK(border >= 0 && border <= CS_MAX_BORDER, -2, "cssim: border %d outside 0..%d", border, CS_MAX_BORDER);
    HRN_CHECK((size_t)H * W <= 0x7fffffffu, -2, "cssim: a frame of %d x %d exceeds 2^31 pixels", H, W);
    HRN_CHECK(p.tiles <= 0x7fffffffu && p.runs <= 0x7fffffffu, -2, "cssim: %zu tiles exceed the grid limit", p.tiles);
    Taps tp;
    float cov_norm = 1.f, tap_excess = 0.f;     // tap_excess: (the sum of the definition's taps)^2 - 1, so that G m = 1 + tap_excess - G(1 - m)
    if (p.T == 7) {
        for (int i = 0; i < CS_MAX_TAPS; ++i) tp.w[i] = i < 7 ? (float)(1.0 / 7.0) : 0.f;
        cov_norm = (float)(49.0 / 48.0);
    } else {
        double g[CS_MAX_TAPS], sum = 0.0;
        for (int i = 0; i < 11; ++i) { const double x = i - 5; g[i] = exp(-x * x / (2.0 * 1.5 * 1.5)); sum += g[i]; }
        double held = 0.0;
        for (int i = 0; i < 11; ++i) { tp.w[i] = (float)(g[i] / sum); held += (double)tp.w[i]; }
        tap_excess = (float)(held * held - 1.0);                // the definition's taps are these fp32 values: -2.8e-9.  1/7 x 7 is 1
    }
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    double* pre = (double*)((char*)workspace + p.pre);
    double* nbias = (double*)((char*)workspace + p.nbias);
    double* partial = nbias + (size_t)B * p.nk * 2;
    const double pix = (double)B * H * W, maps_pix = (double)B * (H - 2 * border - p.T + 1) * (W - 2 * border - p.T + 1);
    {
        HrnProfScope prof("cssim_pre", 4.0 * pix * p.nk, 12.0 * pix, stream);
        hipLaunchKernelGGL(cssim_pre_kernel, dim3((unsigned)p.runs, B), dim3(256), 0, stream, srs, hrs, maps, H, W, border, clip, pre);
        HRN_LAUNCH_CHECK();
        hipLaunchKernelGGL(cssim_pre_finish_kernel, dim3(B), dim3(256), 0, stream, (const double*)pre, (int)p.runs, (int)p.nk, correct_bias,
                           nbias);
        HRN_LAUNCH_CHECK();
    }
    {
        // per map pixel and offset: three fields x two passes x T multiply-adds, and about 40 operations of the SSIM itself
        HrnProfScope prof("cssim_tile", maps_pix * p.nk * (12.0 * p.T + 40.0), 12.0 * pix, stream);
        int rc = p.T == 7 ? launch_tile<7>(srs, hrs, maps, nbias, B, H, W, border, clip, p, tp, cov_norm, c1, c2, tap_excess, partial, stream)
                          : launch_tile<11>(srs, hrs, maps, nbias, B, H, W, border, clip, p, tp, cov_norm, c1, c2, tap_excess, partial, stream);
        if (rc) return rc;
    }
    {
        HrnProfScope prof("cssim_finish", 0.0, 32.0 * B * p.tiles * p.nk, stream);
        const double inv = 1.0 / ((double)(H - 2 * border - p.T + 1) * (double)(W - 2 * border - p.T + 1));
        hipLaunchKernelGGL(cssim_finish_kernel, dim3(B), dim3(256), 0, stream, (const double*)partial, (const double*)nbias, (int)p.tiles,
                           (int)p.nk, inv, out, stats, scores);
        HRN_LAUNCH_CHECK();
    }
    return 0;
}
