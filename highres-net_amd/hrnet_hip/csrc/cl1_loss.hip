// The shift-searched, brightness-corrected L1 (cMAE) and its smooth form, Charbonnier, as a differentiable training tail (DESIGN.md
// section 7m; the project's own definition, restated in fp64 by tests/cl1_ref.py), over shift_loss.hip's crops and offsets.
// With beta = border, h = H - 2 beta, w = W - 2 beta, s = the centre crop of sr, and for the offset k = u (2 beta + 1) + v
//   g = hr[u:u+h, v:v+w], m = map[u:u+h, v:v+w] (a weight), rho(e) = |e| (eps == 0) or sqrt(e^2 + eps^2):
//   n_k = sum m, b_k = sum m (g - s) / n_k, e = s + b_k - g, cL1_k = sum m rho(e) / n_k, sigma_k = sum m rho'(e) / n_k
// and k* = the lowest k of minimal cL1_k among the offsets with n_k > 0.  The gradient goes through k* alone, the bias attached:
//   d out / d sr[beta + y, beta + x] = m*[y, x] / n* (rho'(e*[y, x]) - sigma*)
//
// |s + b_k - g| does not expand into sums that are free of b_k as the square does, so the forward walks the offsets twice.  Both walks
// are shift_loss.hip's: a workgroup owns a 32 x 128 tile of one sample's centre crop, stages that tile of hr and map plus the 2 beta halo
// in LDS once, keeps its 16 sr pixels per thread in registers and, for a row offset u, reads the 4 + 2 beta floats under a lane's four
// pixels as 16-byte reads (16-lane groups on 16 different 16-byte slots of one tile row: conflict-free) and takes every column offset
// from those registers.  The pre-pass sums m and m (g - s) per tile and offset, a finish turns them into {n_k, b_k}; the main pass stages
// the same tile again (from L2 / Infinity Cache), forms e in fp64 from the fp64 bias - so that its sign is the restatement's - and sums
// m rho(e) and m rho'(e); the last finish picks k*.  Tiles are added in a fixed order (runs of tiles in parallel, the runs in order), no
// floating-point atomics: the result is bit-reproducible and a sample's does not depend on its batch.
#include "kernels.h"
#include "wave_sums.h"

namespace {

constexpr int CL_TW = 128;          // tile width: 32 lanes x 4 pixels
constexpr int CL_RPT = 4;           // crop rows per thread
constexpr int CL_TH = 8 * CL_RPT;   // tile height: 8 thread rows x CL_RPT
constexpr int CL_MAX_BORDER = 8;
constexpr int CL_PRE = 0, CL_ABS = 1, CL_CHARB = 2;      // what a walk sums: {m, m (g - s)} | {m |e|, m sign e} | {m rho(e), m rho'(e)}

// 1 / sqrt(q) for rho = q / sqrt(q), rho' = e / sqrt(q): the fp32 estimate and one Newton step in fp64 (1.5 (2^-23)^2 relative) where
// q is an ordinary fp32 number, fp64's own otherwise.
__device__ __forceinline__ double cl1_rsqrt(double q) {
    const float qf = (float)q;
    if (qf >= 1.17549435e-38f && qf <= 3.40282347e38f) {
        const double r = (double)rsqrtf(qf);
        return r * fma(-0.5 * q, r * r, 1.5);
    }
    return 1.0 / sqrt(q);
}

// grid (tiles, B).  partial [B][tiles][(2 beta + 1)^2][2]: the tile's two sums of PHASE at every offset.  nbias [B][(2 beta + 1)^2][2] =
// {n_k, b_k}, read by the main passes only.
template <int BETA, int PHASE>
__global__ __launch_bounds__(256) void cl1_walk_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                       const float* __restrict__ maps, int H, int W, int clip, int ntx,
                                                       const double* __restrict__ nbias, double eps2, double* __restrict__ partial) {
    constexpr int NB = 2 * BETA + 1;
    constexpr int NQ = (4 + 2 * BETA + 3) / 4;          // 16-byte reads that cover a lane's 4 + 2 beta floats
    constexpr int STRIDE = CL_TW - 4 + 4 * NQ;          // the last lane's span ends the row; a multiple of 4 floats
    constexpr int ROWS = CL_TH + 2 * BETA;
    constexpr int NV = 2 * NB, P = pow2_ceil(NV);
    __shared__ __attribute__((aligned(16))) float lg[ROWS * STRIDE];
    __shared__ __attribute__((aligned(16))) float lm[ROWS * STRIDE];
    __shared__ double red[4][P];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = tid & 31, ly = tid >> 5;
    const int tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * CL_TH, x0 = tx * CL_TW;         // the tile's origin: crop coordinates == hr coordinates at offset (0, 0)
    const int h = H - 2 * BETA, w = W - 2 * BETA;
    const size_t img = (size_t)blockIdx.y * H * W;
    const float* sr = srs + img;
    const float* hr = hrs + img;
    const float* mp = maps + img;

    // staging, eight rounds of loads in flight before the first LDS write (a workgroup has one wave per SIMD)
    constexpr int NST = ROWS * STRIDE, DEPTH = 8;
    for (int i0 = tid; i0 < NST; i0 += 256 * DEPTH) {
        float gv[DEPTH], mv[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const int i = i0 + 256 * k;
            const int rr = i / STRIDE, cc = i - rr * STRIDE;
            const int Y = y0 + rr, X = x0 + cc;
            const bool in = i < NST && Y < H && X < W;
            const size_t j = (size_t)Y * W + X;
            gv[k] = in ? hr[j] : 0.f;
            mv[k] = in ? mp[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const int i = i0 + 256 * k;
            if (i < NST) { lg[i] = gv[k]; lm[i] = mv[k]; }
        }
    }
    float s[CL_RPT][4];
    unsigned valid = 0;
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = y0 + ly + 8 * r, x = x0 + 4 * lx + j;
            const bool in = y < h && x < w;
            float t = in ? sr[(size_t)(y + BETA) * W + (x + BETA)] : 0.f;
            if (clip) t = t != t ? t : fminf(fmaxf(t, 0.f), 1.f);       // torch.clamp keeps NaN; fminf / fmaxf alone turn it into 0
            s[r][j] = t;
            valid |= (unsigned)in << (4 * r + j);
        }
    __syncthreads();

    const double* nb = nbias + (size_t)blockIdx.y * (NB * NB * 2);
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + tile) * (NB * NB * 2);
#pragma unroll 1
    for (int u = 0; u < NB; ++u) {
        double bk[NB];                                   // the sample's bias at this row of offsets: uniform over the workgroup
#pragma unroll
        for (int v = 0; v < NB; ++v) bk[v] = PHASE == CL_PRE ? 0.0 : nb[2 * (u * NB + v) + 1];
        double a[P];
#pragma unroll
        for (int i = 0; i < P; ++i) a[i] = 0.0;
#pragma unroll
        for (int r = 0; r < CL_RPT; ++r) {
            const int base = (ly + 8 * r + u) * STRIDE + 4 * lx;
            float g[4 * NQ], m[4 * NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                f32x4 gv = *reinterpret_cast<const f32x4*>(&lg[base + 4 * q]);
                f32x4 mv = *reinterpret_cast<const f32x4*>(&lm[base + 4 * q]);
                asm volatile("" : "+v"(gv), "+v"(mv));      // keep the reads whole (ds_read_b128): unused lanes would split them
                g[4 * q] = gv.x; g[4 * q + 1] = gv.y; g[4 * q + 2] = gv.z; g[4 * q + 3] = gv.w;
                m[4 * q] = mv.x; m[4 * q + 1] = mv.y; m[4 * q + 2] = mv.z; m[4 * q + 3] = mv.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((valid >> (4 * r + j)) & 1)) continue;
                const double sd = (double)s[r][j];
#pragma unroll
                for (int v = 0; v < NB; ++v) {
                    const double mm = (double)m[j + v], gd = (double)g[j + v];
                    if constexpr (PHASE == CL_PRE) {
                        a[2 * v] += mm;
                        a[2 * v + 1] = fma(mm, gd - sd, a[2 * v + 1]);
                    } else {
                        const double e = (sd + bk[v]) - gd;
                        if constexpr (PHASE == CL_ABS) {
                            a[2 * v] = fma(mm, fabs(e), a[2 * v]);
                            a[2 * v + 1] += e > 0.0 ? mm : e < 0.0 ? -mm : 0.0;
                        } else {
                            const double q = fma(e, e, eps2), ri = cl1_rsqrt(q);
                            a[2 * v] = fma(mm, q * ri, a[2 * v]);
                            a[2 * v + 1] = fma(mm, e * ri, a[2 * v + 1]);
                        }
                    }
                }
            }
        }
        WaveSums<P, 0>::run(a, lane);
        const int idx = wave_sums_index<P>(lane);
        __syncthreads();                                 // the previous offset row's readers of `red` are done
        if (lane < P) red[wave][idx] = a[0];
        __syncthreads();
        if (tid < NV) out[u * NV + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

constexpr int CL_FIN_THREADS = 1024;
constexpr int CL_MAXK = (2 * CL_MAX_BORDER + 1) * (2 * CL_MAX_BORDER + 1);

// Adds a sample's tiles in a fixed order: the tiles are cut into as many runs as fit the workgroup, a thread adds one run of one sum with
// eight loads in flight into acc[run * nv + value].  -> the number of runs, which the caller adds in order after a barrier.
__device__ __forceinline__ int cl1_sum_runs(const double* __restrict__ p, int ntiles, int nv, double* acc) {
    const int tid = threadIdx.x;
    int runs = CL_FIN_THREADS / nv;                      // nv <= 578
    if (runs > ntiles) runs = ntiles;
    const int per = (ntiles + runs - 1) / runs;
    if (tid < runs * nv) {
        const int run = tid / nv, val = tid - run * nv;
        const int t0 = run * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
        double sum = 0.0;
        int t = t0;
        for (; t + 8 <= t1; t += 8) {
            double x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = p[(size_t)(t + q) * nv + val];
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += x[q];
        }
        for (; t < t1; ++t) sum += p[(size_t)t * nv + val];
        acc[tid] = sum;
    }
    return runs;
}

// grid (B), 1024 threads.  The pre-pass's tiles -> nbias [B][nk][2] = {n_k, b_k} (b_k = 0 where n_k is not positive).
__global__ __launch_bounds__(CL_FIN_THREADS) void cl1_bias_kernel(const double* __restrict__ partial, int ntiles, int nk,
                                                                  double* __restrict__ nbias) {
    __shared__ double acc[CL_FIN_THREADS];
    const int b = blockIdx.x, nv = 2 * nk;
    const int runs = cl1_sum_runs(partial + (size_t)b * ntiles * nv, ntiles, nv, acc);
    __syncthreads();
    for (int k = threadIdx.x; k < nk; k += CL_FIN_THREADS) {
        double s0 = 0.0, s1 = 0.0;
        for (int r = 0; r < runs; ++r) {
            s0 += acc[r * nv + 2 * k];
            s1 += acc[r * nv + 2 * k + 1];
        }
        double* o = nbias + ((size_t)b * nk + k) * 2;
        o[0] = s0;
        o[1] = s0 > 0.0 ? s1 / s0 : 0.0;
    }
}

// grid (B), 1024 threads.  The main pass's tiles -> cL1_k and sigma_k, the lowest k of minimal cL1_k among n_k > 0 (a NaN is never taken
// over a number), out [B] and stats [B][5] = {n*, b*, cL1*, k*, sigma*}.
__global__ __launch_bounds__(CL_FIN_THREADS) void cl1_finish_kernel(const double* __restrict__ partial, const double* __restrict__ nbias,
                                                                    int ntiles, int nk, float* __restrict__ out, double* __restrict__ stats) {
    __shared__ double acc[CL_FIN_THREADS];
    __shared__ double cn[CL_MAXK], cl[CL_MAXK], cs[CL_MAXK];
    const int b = blockIdx.x, nv = 2 * nk;
    const int runs = cl1_sum_runs(partial + (size_t)b * ntiles * nv, ntiles, nv, acc);
    __syncthreads();
    const double* nb = nbias + (size_t)b * nk * 2;
    for (int k = threadIdx.x; k < nk; k += CL_FIN_THREADS) {
        double s0 = 0.0, s1 = 0.0;
        for (int r = 0; r < runs; ++r) {
            s0 += acc[r * nv + 2 * k];
            s1 += acc[r * nv + 2 * k + 1];
        }
        const double n = nb[2 * k];
        cn[k] = n; cl[k] = s0 / n; cs[k] = s1 / n;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best = -1;
    for (int k = 0; k < nk; ++k)
        if (cn[k] > 0.0 && (best < 0 || cl[k] < cl[best] || (cl[best] != cl[best] && cl[k] == cl[k]))) best = k;
    double* st = stats + 5 * (size_t)b;
    if (best < 0) {                                      // no clear pixel at any offset: NaN, and the backward writes zeros
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        st[0] = 0.0; st[1] = 0.0; st[2] = nan; st[3] = -1.0; st[4] = 0.0;
        out[b] = __int_as_float(0x7fc00000);
        return;
    }
    st[0] = cn[best]; st[1] = nb[2 * best + 1]; st[2] = cl[best]; st[3] = (double)best; st[4] = cs[best];
    out[b] = (float)cl[best];
}

// grid (rows of blocks, B): one elementwise pass over all of d_srs, the border frame and clamped pixels written as zeros.  e is formed in
// fp64 from the fp64 bias, as the forward forms it: the sign of the L1 gradient depends on it.
__global__ __launch_bounds__(256) void cl1_backward_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                           const float* __restrict__ maps, const double* __restrict__ stats,
                                                           const float* __restrict__ d_out, int H, int W, int border, int clip, double eps2,
                                                           float* __restrict__ d_srs) {
    const int b = blockIdx.y;
    const double cnt = stats[5 * b + 0], bias = stats[5 * b + 1], sigma = stats[5 * b + 4];
    const int k = (int)stats[5 * b + 3];
    const int nb = 2 * border + 1;
    const bool none = !(cnt > 0.0) || k < 0 || k >= nb * nb;     // no clear pixel (or stats of another border): zeros, nothing read out of bounds
    const int u = none ? 0 : k / nb, v = none ? 0 : k - (k / nb) * nb;
    const double coef = none ? 0.0 : (double)d_out[b] / cnt;
    const size_t n = (size_t)H * W, base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int Y = (int)(i / W), X = (int)(i - (size_t)Y * W);
        float grad = 0.f;
        if (!none && Y >= border && Y < H - border && X >= border && X < W - border) {
            const float s = srs[base + i];
            if (!clip || (s >= 0.f && s <= 1.f)) {       // torch.clamp passes the gradient on [min, max], ends included
                const size_t j = base + (size_t)(Y - border + u) * W + (X - border + v);
                const double e = ((double)s + bias) - (double)hrs[j];
                const double dr = eps2 > 0.0 ? e / sqrt(fma(e, e, eps2)) : e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : e;    // e: 0, or NaN
                grad = (float)(coef * (double)maps[j] * (dr - sigma));
            }
        }
        d_srs[base + i] = grad;
    }
}

template <int PHASE>
void launch_walk(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, int ntx, int ntiles,
                 const double* nbias, double eps2, double* partial, hipStream_t stream) {
#define CL1_WALK(BETA)                                                                                                                  \
    case BETA:                                                                                                                          \
        hipLaunchKernelGGL((cl1_walk_kernel<BETA, PHASE>), dim3(ntiles, B), dim3(256), 0, stream, srs, hrs, maps, H, W, clip, ntx, nbias, \
                           eps2, partial);                                                                                              \
        break;
    switch (border) {
        CL1_WALK(0) CL1_WALK(1) CL1_WALK(2) CL1_WALK(3) CL1_WALK(4) CL1_WALK(5) CL1_WALK(6) CL1_WALK(7) CL1_WALK(8)
    }
#undef CL1_WALK
}

size_t tiles_of(int H, int W, int border, int* ntx) {
    const int h = H - 2 * border, w = W - 2 * border;
    const int nx = (w + CL_TW - 1) / CL_TW, ny = (h + CL_TH - 1) / CL_TH;
    if (ntx) *ntx = nx;
    return (size_t)nx * ny;
}

size_t nk_of(int border) { return (size_t)(2 * border + 1) * (2 * border + 1); }

}  // namespace

// the tiles' sums (one buffer, used by the pre-pass and then by the main pass) and nbias
size_t hrn_cl1_loss_workspace_bytes_impl(int B, int H, int W, int border) {
    return (size_t)B * (tiles_of(H, W, border, nullptr) + 1) * nk_of(border) * 2 * sizeof(double);
}

int hrn_launch_cl1_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, float eps,
                              float* out, double* stats, double* workspace, hipStream_t stream) {
    HRN_CHECK(border >= 0 && border <= CL_MAX_BORDER, -2, "cl1 loss: border %d outside 0..%d", border, CL_MAX_BORDER);
    int ntx = 0;
    const size_t tiles = tiles_of(H, W, border, &ntx);
    HRN_CHECK(tiles <= 0x7fffffffu, -2, "cl1 loss: %zu tiles exceed the grid limit", tiles);
    const int ntiles = (int)tiles, nk = (int)nk_of(border);
    double* partial = workspace;
    double* nbias = workspace + (size_t)B * tiles * nk * 2;
    const double eps2 = (double)eps * (double)eps;
    HrnProfScope prof("cl1_fwd", 0.0, 24.0 * B * H * W, stream);
    launch_walk<CL_PRE>(srs, hrs, maps, B, H, W, border, clip, ntx, ntiles, nbias, 0.0, partial, stream);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl1_bias_kernel, dim3(B), dim3(CL_FIN_THREADS), 0, stream, (const double*)partial, ntiles, nk, nbias);
    HRN_LAUNCH_CHECK();
    if (eps == 0.f) launch_walk<CL_ABS>(srs, hrs, maps, B, H, W, border, clip, ntx, ntiles, nbias, 0.0, partial, stream);
    else launch_walk<CL_CHARB>(srs, hrs, maps, B, H, W, border, clip, ntx, ntiles, nbias, eps2, partial, stream);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl1_finish_kernel, dim3(B), dim3(CL_FIN_THREADS), 0, stream, (const double*)partial, (const double*)nbias, ntiles, nk,
                       out, stats);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_cl1_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                 int H, int W, int border, int clip, float eps, float* d_srs, hipStream_t stream) {
    HrnProfScope prof("cl1_bwd", 0.0, 16.0 * B * H * W, stream);
    size_t gx = ((size_t)H * W + 1023) / 1024;          // four pixels per thread
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(cl1_backward_kernel, dim3((unsigned)gx, B), dim3(256), 0, stream, srs, hrs, maps, stats, d_out, H, W, border, clip,
                       (double)eps * (double)eps, d_srs);
    HRN_LAUNCH_CHECK();
    return 0;
}
