// The gradient of cSSIM (cssim.hip; the definition is in include/hrnet_hip.h) with respect to srs, through the one
// offset k* the forward selected and with the brightness bias attached.  Per map pixel, with a = mu_x, c = mu_y:
//   A1 = 2ac + C1, B1 = a^2 + c^2 + C1, A2 = 2 v_xy + C2, B2 = v_x + v_y + C2,
//   S_c = dSSIM/dc = 2 A2 (a - c) (a (a + c) + C1) / (B1^2 B2)      (= 2a A2/(B1 B2) - 2c A1 A2/(B1^2 B2), without its cancellation)
//   beta = 2 cov_norm S_vy = -2 cov_norm A1 A2 / (B1 B2^2),   gamma = cov_norm S_vxy = 2 cov_norm A1 / (B1 B2),
//   alpha = S_c - beta c - gamma a,        D_q = (G^T alpha)_q + Y_q (G^T beta)_q + X_q (G^T gamma)_q
// G^T the adjoint of the "valid" window: the map-sized field, zero outside the map, correlated with the flipped taps back onto the crop.
// As in the forward the fields are centred per tile, kappa = the mean of g over the clear pixels the tile staged:
//   X~ = m (g - kappa),  Y~ = m (s + b - kappa),  w = 1 - G m,
//   alpha' = S_c - beta (G Y~ - kappa w) - gamma (G X~ - kappa w),      D_q = G^T alpha' + Y~_q G^T beta + X~_q G^T gamma   where m_q = 1
// (a masked q gets another value, which nothing reads: the gradient and the mean below carry the factor m_q).  a - c = G X~ - G Y~ exactly.
//
//   cssim_bwd_tile_kernel<T>   a workgroup owns 16 x (64 - 2 (T - 1)) crop pixels of one sample.  It stages s, g, m at k* with a halo of
//                              2 (T - 1) (64 window columns) as Y~, X~ and bytes, filters {1 - m, X~, X~^2} and then {Y~, Y~^2, X~Y~}
//                              with the forward's two sliding passes (pass 1 down the columns, a lane per window column and 4 map
//                              rows per run; pass 2 along the rows out of the stride-65 layout, 4 map pixels per lane), forms alpha',
//                              beta, gamma per map pixel in fp32 (0 outside the map), filters the three back with the same two passes
//                              and the flipped taps, and writes the raw D into d_srs' crop and its waves' fp64 sums of m D to `sums`.
//   cssim_bwd_mean_kernel      per sample M = sum m D / n*: 256 runs of the tiles' sums in index order, the runs in index order.
//   cssim_bwd_finish_kernel    d_srs = d_out[b] pass m (D - M) / Np on the crop, 0 on the border frame and for a sample with k* < 0.
// No atomics; the sums' order depends on the frame's shape alone: two runs give the same bits, a sample's gradient does not depend on
// its batch.  The border is a run-time argument: one offset is walked, so no row stride depends on it.
#include "kernels.h"
#include "wave_sums.h"
#include <math.h>

#pragma clang fp contract(off)      // every fused multiply-add is written out

namespace {

constexpr int CB_MAX_TAPS = 11;
constexpr int CB_WIN = 64;          // window columns of a tile: one lane per column in pass 1
constexpr int CB_OR = 16;           // crop rows of a tile
constexpr int CB_RUN = 4;           // rows per lane and run in pass 1, pixels per lane in pass 2
constexpr int CB_VS = CB_WIN + 1;   // row stride of the pass-1 output: odd
constexpr int CB_FIN_PIX = 4;       // pixels per thread of the finish

struct Taps { float w[CB_MAX_TAPS]; };

// A tile: OR x OC crop pixels <- MR x MC map pixels <- IR x 64 staged pixels; the map's rows are walked in NRUN runs of 4.
struct Geo { int halo, ir, mr, mc, oc, nrun, irp, mcs; };
__host__ __device__ constexpr Geo cb_geo(int T) {
    Geo g = {0, 0, 0, 0, 0, 0, 0, 0};
    g.halo = T - 1;
    g.ir = CB_OR + 2 * g.halo;
    g.mr = CB_OR + g.halo;
    g.mc = CB_WIN - g.halo;
    g.oc = g.mc - g.halo;
    g.nrun = (g.mr + CB_RUN - 1) / CB_RUN;
    g.irp = g.nrun * CB_RUN + g.halo;           // the last run reads rows past IR: staged as zeros
    g.mcs = g.mc + ((1 - g.mc) & 3);            // row stride of the map fields: 1 mod 4
    return g;
}

// the LDS of a tile, in floats: X~ | Y~ | V (3 fields of pass 1) | A (3 map fields) | M (bytes)
struct TileLds { int x, y, v, a, m, total, vf; };
__host__ __device__ constexpr TileLds cb_lds(int T) {
    const Geo g = cb_geo(T);
    TileLds l = {0, 0, 0, 0, 0, 0, 0};
    l.x = 0;
    l.y = l.x + g.irp * CB_WIN;
    l.v = l.y + g.irp * CB_WIN;
    l.vf = g.nrun * CB_RUN * CB_VS;             // a field of V
    l.a = l.v + 3 * l.vf + 16;                  // pass 2's lanes past a row's last pixel read up to T + 2 floats past its end: the pad
    l.m = l.a + 3 * g.mr * g.mcs;
    l.total = l.m + (g.irp * CB_WIN + 3) / 4;
    return l;
}

// grid (tiles, B), dynamic LDS cb_lds(T).total floats.  sums [B][tiles][4 waves] = the wave's sum of m D.
template <int T>
__global__ __launch_bounds__(256) void cssim_bwd_tile_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                             const float* __restrict__ maps, const double* __restrict__ stats, int H, int W,
                                                             int border, int clip, int ntx, Taps tp, float cov_norm, float c1, float c2,
                                                             float tap_excess, float* __restrict__ d_srs, double* __restrict__ sums) {
    constexpr Geo GEO = cb_geo(T);
    constexpr TileLds L = cb_lds(T);
    constexpr int HALO = GEO.halo, IRP = GEO.irp, MR = GEO.mr, MC = GEO.mc, OC = GEO.oc, NRUN = GEO.nrun, MCS = GEO.mcs;
    constexpr int NIN = CB_RUN + T - 1, VF = L.vf, AF = MR * MCS;
    static_assert(L.total * sizeof(float) <= 65536, "a tile's LDS fits what a launch gets without opting in");
    static_assert(CB_OR == 4 * CB_RUN && CB_OR * (CB_WIN / CB_RUN) == 256, "the adjoint's passes are one round of the workgroup");
    static_assert(CB_WIN - CB_RUN + NIN - 1 < CB_VS + 16, "pass 2's reads past a row stay inside the pad");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* X = lds + L.x;
    float* Y = lds + L.y;
    float* V = lds + L.v;
    float* A = lds + L.a;
    unsigned char* M = reinterpret_cast<unsigned char*>(lds + L.m);

    const double* st = stats + 4 * (size_t)blockIdx.y;
    const int k = (int)st[3], nb = 2 * border + 1;
    if (k < 0 || k >= nb * nb) return;                              // no eligible offset: the finish writes the sample's zeros
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = k / nb, v = k - u * nb;
    const int h = H - 2 * border, w = W - 2 * border, mh = h - T + 1, mw = w - T + 1;
    const int tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * CB_OR, x0 = tx * OC;                        // the tile's first crop pixel; staged row r is crop row y0 - HALO + r
    const size_t img = (size_t)blockIdx.y * H * W;
    const float* sr = srs + img;
    const float* hr = hrs + img;
    const float* mp = maps + img;

    // ---- stage s, g, m at k*; outside the crop 0, which feeds only map pixels outside the map
    for (int i = tid; i < IRP * CB_WIN; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int y = y0 - HALO + r, x = x0 - HALO + c;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        float s = 0.f, g = 0.f;
        bool m = false;
        if (in) {
            const size_t j = (size_t)(y + u) * W + (x + v);
            s = sr[(size_t)(y + border) * W + (x + border)];
            g = hr[j];
            m = mp[j] != 0.f;
        }
        if (clip) s = s != s ? s : fminf(fmaxf(s, 0.f), 1.f);
        Y[i] = s;
        X[i] = g;
        M[i] = m;
    }
    __syncthreads();

    // ---- the tile's centre kappa, as the forward takes it: the same bits in every thread
    float cen;
    {
        float n = 0.f, sg = 0.f;
        for (int i = tid; i < IRP * CB_WIN; i += 256) {
            const float m = (float)M[i];
            n += m;
            sg = fmaf(m, X[i], sg);
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
    {
        const float cs = (float)((double)cen - st[1]);              // Y~ = m (s - (kappa - b))
        for (int i = tid; i < IRP * CB_WIN; i += 256) {             // a thread rewrites what it alone reads here
            const float m = (float)M[i];
            X[i] = m * (X[i] - cen);
            Y[i] = m * (Y[i] - cs);
        }
    }
    __syncthreads();

    // ---- the six map fields in two groups of three: f = 0 {1 - m, X~, X~^2}, f = 1 {Y~, Y~^2, X~ Y~}
    for (int f = 0; f < 2; ++f) {
        for (int run = wave; run < NRUN; run += 4) {                // pass 1: window column `lane`, map rows 4 run ..
            float p0[NIN], p1[NIN], p2[NIN];
            const int i0 = run * CB_RUN * CB_WIN + lane;
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const float x = X[i0 + i * CB_WIN];
                if (f == 0) {
                    p0[i] = 1.f - (float)M[i0 + i * CB_WIN]; p1[i] = x; p2[i] = x * x;
                } else {
                    const float y = Y[i0 + i * CB_WIN];
                    p0[i] = y; p1[i] = y * y; p2[i] = x * y;
                }
            }
            float* Vp = V + run * CB_RUN * CB_VS + lane;
#pragma unroll
            for (int j = 0; j < CB_RUN; ++j) {
                float a0 = tp.w[0] * p0[j], a1 = tp.w[0] * p1[j], a2 = tp.w[0] * p2[j];
#pragma unroll
                for (int o = 1; o < T; ++o) {
                    a0 = fmaf(tp.w[o], p0[j + o], a0);
                    a1 = fmaf(tp.w[o], p1[j + o], a1);
                    a2 = fmaf(tp.w[o], p2[j + o], a2);
                }
                Vp[j * CB_VS] = a0;
                Vp[VF + j * CB_VS] = a1;
                Vp[2 * VF + j * CB_VS] = a2;
            }
        }
        __syncthreads();
        for (int item = tid; item < MR * (CB_WIN / CB_RUN); item += 256) {     // pass 2: map row item / 16, map columns 4 (item % 16) ..
            const int py = item >> 4, px = CB_RUN * (item & 15);
            float q0[NIN], q1[NIN], q2[NIN];
            const float* Vq = V + py * CB_VS + px;
#pragma unroll
            for (int i = 0; i < NIN; ++i) { q0[i] = Vq[i]; q1[i] = Vq[VF + i]; q2[i] = Vq[2 * VF + i]; }
            const int gy = y0 - HALO + py;                          // the map pixel's row in the map
#pragma unroll
            for (int j = 0; j < CB_RUN; ++j) {
                float f0 = tp.w[0] * q0[j], f1 = tp.w[0] * q1[j], f2 = tp.w[0] * q2[j];
#pragma unroll
                for (int o = 1; o < T; ++o) {
                    f0 = fmaf(tp.w[o], q0[j + o], f0);
                    f1 = fmaf(tp.w[o], q1[j + o], f1);
                    f2 = fmaf(tp.w[o], q2[j + o], f2);
                }
                if (px + j >= MC) continue;                         // the lanes past the tile's last map column own nothing
                const int a = py * MCS + px + j;
                if (f == 0) {
                    const float wm = f0 - tap_excess, ax = f1, axx = f2;
                    const float cw = cen * wm, e = (cen * (1.f - wm)) * cw;
                    A[a] = wm;
                    A[AF + a] = ax;
                    A[2 * AF + a] = cov_norm * (fmaf(2.f * cw, ax, fmaf(-ax, ax, axx)) + e);
                    continue;
                }
                const int gx = x0 - HALO + px + j;
                const bool ok = gy >= 0 && gy < mh && gx >= 0 && gx < mw;
                const float wm = A[a], ax = A[AF + a], vx = A[2 * AF + a];         // written by this thread in the first group
                const float ay = f0, ayy = f1, axy = f2;
                const float cp = cen * (1.f - wm), cw = cen * wm, e = cp * cw;
                const float mux = ax + cp, muy = ay + cp;
                const float vy = cov_norm * (fmaf(2.f * cw, ay, fmaf(-ay, ay, ayy)) + e);
                const float vxy = cov_norm * (fmaf(cw, ax + ay, fmaf(-ax, ay, axy)) + e);
                const float a1 = fmaf(2.f * mux, muy, c1), b1 = fmaf(mux, mux, fmaf(muy, muy, c1));
                const float a2 = fmaf(2.f, vxy, c2), b2 = (vx + vy) + c2;
                const float i1 = 1.f / b1, i2 = 1.f / b2;           // IEEE division
                const float r1 = a1 * i1, r2 = a2 * i2;
                const float sc = ((2.f * r2) * (ax - ay)) * (fmaf(mux, mux + muy, c1) * (i1 * i1));
                const float beta = (-2.f * cov_norm) * ((r1 * i2) * r2);
                const float gamma = (2.f * cov_norm) * (r1 * i2);
                const float alpha = fmaf(-gamma, ax - cw, fmaf(-beta, ay - cw, sc));
                A[a] = ok ? alpha : 0.f;
                A[AF + a] = ok ? beta : 0.f;
                A[2 * AF + a] = ok ? gamma : 0.f;
            }
        }
        __syncthreads();
    }

    // ---- the adjoint: D(i) = sum_o w[T - 1 - o] field(i + o), down the map's columns, then along its rows
    {
        float p0[NIN], p1[NIN], p2[NIN];
        const int col = lane < MC ? lane : MC - 1;                 // the lanes past the map's last column repeat it; nothing reads their output
        const float* Ap = A + CB_RUN * wave * MCS + col;
#pragma unroll
        for (int i = 0; i < NIN; ++i) { p0[i] = Ap[i * MCS]; p1[i] = Ap[AF + i * MCS]; p2[i] = Ap[2 * AF + i * MCS]; }
        float* Vp = V + CB_RUN * wave * CB_VS + lane;
#pragma unroll
        for (int j = 0; j < CB_RUN; ++j) {
            float a0 = tp.w[T - 1] * p0[j], a1 = tp.w[T - 1] * p1[j], a2 = tp.w[T - 1] * p2[j];
#pragma unroll
            for (int o = 1; o < T; ++o) {
                a0 = fmaf(tp.w[T - 1 - o], p0[j + o], a0);
                a1 = fmaf(tp.w[T - 1 - o], p1[j + o], a1);
                a2 = fmaf(tp.w[T - 1 - o], p2[j + o], a2);
            }
            Vp[j * CB_VS] = a0;
            Vp[VF + j * CB_VS] = a1;
            Vp[2 * VF + j * CB_VS] = a2;
        }
    }
    __syncthreads();
    double sum = 0.0;
    {
        const int py = CB_RUN * wave + (lane >> 4), px = CB_RUN * (lane & 15);    // crop row y0 + py, crop columns x0 + px ..
        float q0[NIN], q1[NIN], q2[NIN];
        const float* Vq = V + py * CB_VS + px;
#pragma unroll
        for (int i = 0; i < NIN; ++i) { q0[i] = Vq[i]; q1[i] = Vq[VF + i]; q2[i] = Vq[2 * VF + i]; }
        const int y = y0 + py;
#pragma unroll
        for (int j = 0; j < CB_RUN; ++j) {
            float f0 = tp.w[T - 1] * q0[j], f1 = tp.w[T - 1] * q1[j], f2 = tp.w[T - 1] * q2[j];
#pragma unroll
            for (int o = 1; o < T; ++o) {
                f0 = fmaf(tp.w[T - 1 - o], q0[j + o], f0);
                f1 = fmaf(tp.w[T - 1 - o], q1[j + o], f1);
                f2 = fmaf(tp.w[T - 1 - o], q2[j + o], f2);
            }
            const int x = x0 + px + j;
            if (px + j >= OC || y >= h || x >= w) continue;
            const int i = (py + HALO) * CB_WIN + px + j + HALO;
            const float d = fmaf(X[i], f2, fmaf(Y[i], f1, f0));
            d_srs[img + (size_t)(y + border) * W + (x + border)] = d;
            if (M[i]) sum += (double)d;
        }
    }
    WaveSums<1, 0>::run(&sum, lane);
    if (lane == 0) sums[((size_t)blockIdx.y * gridDim.x + tile) * 4 + wave] = sum;
}

// grid (B).  mean [B] = M: thread t adds its run of the sample's tile sums in index order, thread 0 the 256 runs in index order.
__global__ __launch_bounds__(256) void cssim_bwd_mean_kernel(const double* __restrict__ sums, const double* __restrict__ stats, int nsums,
                                                             int correct_bias, double* __restrict__ mean) {
    __shared__ double part[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* st = stats + 4 * (size_t)b;
    const bool live = correct_bias && st[3] >= 0.0 && st[0] > 0.0;  // uniform over the workgroup; else the sums may be unwritten
    const int per = (nsums + 255) / 256, lo = t * per, hi = min(nsums, lo + per);
    double s = 0.0;
    if (live)
        for (int i = lo; i < hi; ++i) s += sums[(size_t)b * nsums + i];
    part[t] = s;
    __syncthreads();
    if (t != 0) return;
    s = 0.0;
    for (int i = 0; i < 256; ++i) s += part[i];
    mean[b] = live ? s / st[0] : 0.0;
}

// grid (runs of 1024 pixels, B).  In place on d_srs: the crop holds the tile kernel's D.
__global__ __launch_bounds__(256) void cssim_bwd_finish_kernel(const float* __restrict__ srs, const float* __restrict__ maps,
                                                               const double* __restrict__ stats, const double* __restrict__ mean,
                                                               const float* __restrict__ d_out, int H, int W, int border, int clip,
                                                               double inv_np, float* __restrict__ d_srs) {
    const int b = blockIdx.y;
    const double* st = stats + 4 * (size_t)b;
    const int nb = 2 * border + 1, k = st[3] >= 0.0 && st[3] < (double)(nb * nb) ? (int)st[3] : -1;      // anything else: no offset
    const int u = k < 0 ? 0 : k / nb, v = k < 0 ? 0 : k - u * nb;
    const int h = H - 2 * border, w = W - 2 * border;
    const size_t npix = (size_t)H * W, img = (size_t)b * npix;
    const double scale = (double)d_out[b] * inv_np, mv = mean[b];
#pragma unroll
    for (int j = 0; j < CB_FIN_PIX; ++j) {
        const size_t p = ((size_t)blockIdx.x * CB_FIN_PIX + j) * 256 + threadIdx.x;
        if (p >= npix) continue;
        const int yy = (int)(p / W), y = yy - border, x = (int)(p - (size_t)yy * W) - border;
        float out = 0.f;
        if (k >= 0 && y >= 0 && y < h && x >= 0 && x < w) {
            const float s = srs[img + p];
            const bool pass = !clip || (s >= 0.f && s <= 1.f);      // where torch.clamp passes a gradient
            if (pass && maps[img + (size_t)(y + u) * W + (x + v)] != 0.f) out = (float)(((double)d_srs[img + p] - mv) * scale);
        }
        d_srs[img + p] = out;
    }
}

struct Plan { int T, ntx; size_t tiles, sums, total; };
Plan plan_of(int B, int H, int W, int border, int window) {
    Plan p;
    p.T = window == 1 ? 7 : 11;
    const int h = H - 2 * border, w = W - 2 * border, oc = cb_geo(p.T).oc;
    p.ntx = (w + oc - 1) / oc;
    p.tiles = (size_t)p.ntx * ((h + CB_OR - 1) / CB_OR);
    p.sums = (size_t)B * p.tiles * 4 * sizeof(double);
    p.total = p.sums + (size_t)B * sizeof(double);
    return p;
}

template <int T>
int launch_tile(const float* srs, const float* hrs, const float* maps, const double* stats, int B, int H, int W, int border, int clip,
                const Plan& p, const Taps& tp, float cov_norm, float c1, float c2, float tap_excess, float* d_srs, double* sums,
                hipStream_t stream) {
    constexpr int bytes = cb_lds(T).total * (int)sizeof(float);
    hipLaunchKernelGGL((cssim_bwd_tile_kernel<T>), dim3((unsigned)p.tiles, B), dim3(256), bytes, stream, srs, hrs, maps, stats, H, W, border,
                       clip, p.ntx, tp, cov_norm, c1, c2, tap_excess, d_srs, sums);
    HRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

size_t hrn_cssim_loss_backward_workspace_bytes_impl(int B, int H, int W, int border, int window) {
    return plan_of(B, H, W, border, window).total;
}

int hrn_launch_cssim_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                   int H, int W, int border, int window, int clip, int correct_bias, float data_range, float* d_srs,
                                   void* workspace, hipStream_t stream) {
    const Plan p = plan_of(B, H, W, border, window);
    HRN_CHECK((size_t)H * W <= 0x7fffffffu, -2, "cssim backward: a frame of %d x %d exceeds 2^31 pixels", H, W);
    const size_t fin = ((size_t)H * W + 256 * CB_FIN_PIX - 1) / (256 * CB_FIN_PIX);
    HRN_CHECK(p.tiles * 4 <= 0x7fffffffu && fin <= 0x7fffffffu, -2, "cssim backward: %zu tiles exceed the grid limit", p.tiles);
    Taps tp;
    float cov_norm = 1.f, tap_excess = 0.f;     // as hrn_launch_shift_cssim takes them
    if (p.T == 7) {
        for (int i = 0; i < CB_MAX_TAPS; ++i) tp.w[i] = i < 7 ? (float)(1.0 / 7.0) : 0.f;
        cov_norm = (float)(49.0 / 48.0);
    } else {
        double g[CB_MAX_TAPS], sum = 0.0;
        for (int i = 0; i < 11; ++i) { const double x = i - 5; g[i] = exp(-x * x / (2.0 * 1.5 * 1.5)); sum += g[i]; }
        double held = 0.0;
        for (int i = 0; i < 11; ++i) { tp.w[i] = (float)(g[i] / sum); held += (double)tp.w[i]; }
        tap_excess = (float)(held * held - 1.0);
    }
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    double* sums = (double*)workspace;
    double* mean = (double*)((char*)workspace + p.sums);
    const double pix = (double)B * H * W;
    {
        // per crop pixel: nine fields x two passes x T multiply-adds over the tile's halo, and about 60 operations per map pixel
        HrnProfScope prof("cssim_bwd_tile", pix * (36.0 * p.T + 60.0), 16.0 * pix, stream);
        int rc = p.T == 7 ? launch_tile<7>(srs, hrs, maps, stats, B, H, W, border, clip, p, tp, cov_norm, c1, c2, tap_excess, d_srs, sums, stream)
                          : launch_tile<11>(srs, hrs, maps, stats, B, H, W, border, clip, p, tp, cov_norm, c1, c2, tap_excess, d_srs, sums, stream);
        if (rc) return rc;
    }
    {
        HrnProfScope prof("cssim_bwd_finish", 4.0 * pix, 16.0 * pix, stream);
        hipLaunchKernelGGL(cssim_bwd_mean_kernel, dim3(B), dim3(256), 0, stream, (const double*)sums, stats, (int)(p.tiles * 4), correct_bias,
                           mean);
        HRN_LAUNCH_CHECK();
        const double inv_np = 1.0 / ((double)(H - 2 * border - p.T + 1) * (double)(W - 2 * border - p.T + 1));
        hipLaunchKernelGGL(cssim_bwd_finish_kernel, dim3((unsigned)fin, B), dim3(256), 0, stream, srs, maps, stats, (const double*)mean, d_out,
                           H, W, border, clip, inv_np, d_srs);
        HRN_LAUNCH_CHECK();
    }
    return 0;
}
