// The shift-searched, brightness-corrected L1 (cMAE) and its smooth form, Charbonnier, as a differentiable training tail (DESIGN.md
// section 7m; the project's own definition, restated in fp64 by tests/cl1_ref.py), over shift_loss.hip's crops and offsets.
// With beta = border, h = H - 2 beta, w = W - 2 beta, s = the centre crop of sr, and for the offset k = u (2 beta + 1) + v
//   g = hr[u:u+h, v:v+w], m = map[u:u+h, v:v+w] (a weight), rho(e) = |e| (eps == 0) or sqrt(e^2 + eps^2):
//   n_k = sum m, b_k = sum m (g - s) / n_k, e = s + b_k - g, cL1_k = sum m rho(e) / n_k, sigma_k = sum m rho'(e) / n_k
// and k* = the lowest k of minimal cL1_k among the offsets with n_k > 0.  The gradient goes through k* alone, the bias attached:
//   d out / d sr[beta + y, beta + x] = m*[y, x] / n* (rho'(e*[y, x]) - sigma*)
//
// |s + b_k - g| does not expand into sums that are free of b_k as the square does, so the forward walks the offsets twice, both times
// with offset_walk.h's walk of a 32 x 128 tile.  The pre-pass sums m and m (g - s) per tile and offset, a finish turns them into
// {n_k, b_k}; the main pass stages the same tile again (from L2 / Infinity Cache), forms e in fp64 from the fp64 bias - so that its sign
// is the restatement's - and sums m rho(e) and m rho'(e); the last finish picks k*.  Tiles are added in a fixed order (runs of tiles in
// parallel, the runs in order), no floating-point atomics: the result is bit-reproducible and a sample's does not depend on its batch.
#include "offset_walk.h"

namespace {

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

// The two sums of PHASE.  nb [(2 beta + 1)^2][2] = the sample's {n_k, b_k}, read by the main passes only.
template <int PHASE>
struct Cl1Term {
    static constexpr int SUMS = 2;
    const double* nb;
    double eps2;
    template <int NB>
    struct Row { double bk[NB]; };                       // the sample's bias at this row of offsets
    template <int NB>
    __device__ __forceinline__ Row<NB> row(int u) const {
        Row<NB> r;
#pragma unroll
        for (int v = 0; v < NB; ++v) r.bk[v] = PHASE == CL_PRE ? 0.0 : nb[2 * (u * NB + v) + 1];
        return r;
    }
    template <int NB>
    __device__ __forceinline__ void add(const Row<NB>& row, int v, double mm, double sd, double gd, double* a) const {
        if constexpr (PHASE == CL_PRE) {
            a[0] += mm;
            a[1] = fma(mm, gd - sd, a[1]);
        } else {
            const double e = (sd + row.bk[v]) - gd;
            if constexpr (PHASE == CL_ABS) {
                a[0] = fma(mm, fabs(e), a[0]);
                a[1] += e > 0.0 ? mm : e < 0.0 ? -mm : 0.0;
            } else {
                const double q = fma(e, e, eps2), ri = cl1_rsqrt(q);
                a[0] = fma(mm, q * ri, a[0]);
                a[1] = fma(mm, e * ri, a[1]);
            }
        }
    }
};

// grid (tiles, B).  partial [B][tiles][(2 beta + 1)^2][2]: the tile's two sums of PHASE at every offset.  nbias [B][(2 beta + 1)^2][2].
template <int BETA, int PHASE>
__global__ __launch_bounds__(256) void cl1_walk_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                       const float* __restrict__ maps, int H, int W, int clip, int ntx,
                                                       const double* __restrict__ nbias, double eps2, double* __restrict__ partial) {
    constexpr int NB = 2 * BETA + 1;
    offset_walk<BETA>(srs, hrs, maps, H, W, clip, ntx, Cl1Term<PHASE>{nbias + (size_t)blockIdx.y * (NB * NB * 2), eps2}, partial);
}

// grid (B), 1024 threads.  The pre-pass's tiles -> nbias [B][nk][2] = {n_k, b_k} (b_k = 0 where n_k is not positive).
__global__ __launch_bounds__(OW_FIN_THREADS) void cl1_bias_kernel(const double* __restrict__ partial, int ntiles, int nk,
                                                                  double* __restrict__ nbias) {
    __shared__ double acc[OW_FIN_THREADS];
    const int b = blockIdx.x, nv = 2 * nk;
    const int runs = sum_tile_runs(partial + (size_t)b * ntiles * nv, ntiles, nv, acc);
    __syncthreads();
    for (int k = threadIdx.x; k < nk; k += OW_FIN_THREADS) {
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
__global__ __launch_bounds__(OW_FIN_THREADS) void cl1_finish_kernel(const double* __restrict__ partial, const double* __restrict__ nbias,
                                                                    int ntiles, int nk, float* __restrict__ out, double* __restrict__ stats) {
    __shared__ double acc[OW_FIN_THREADS];
    __shared__ double cn[OW_MAXK], cl[OW_MAXK], cs[OW_MAXK];
    const int b = blockIdx.x, nv = 2 * nk;
    const int runs = sum_tile_runs(partial + (size_t)b * ntiles * nv, ntiles, nv, acc);
    __syncthreads();
    const double* nb = nbias + (size_t)b * nk * 2;
    for (int k = threadIdx.x; k < nk; k += OW_FIN_THREADS) {
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

// grid (rows of blocks, B): offset_walk.h's backward pass.  e is formed in fp64 from the fp64 bias, as the forward forms it: the sign of
// the L1 gradient depends on it.
__global__ __launch_bounds__(256) void cl1_backward_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                           const float* __restrict__ maps, const double* __restrict__ stats,
                                                           const float* __restrict__ d_out, int H, int W, int border, int clip, double eps2,
                                                           float* __restrict__ d_srs) {
    offset_walk_backward<5>(srs, hrs, maps, stats, H, W, border, clip, d_srs, [=](const double* st, bool none) {
        const double bias = st[1], sigma = st[4];
        const double coef = none ? 0.0 : (double)d_out[blockIdx.y] / st[0];
        return [=](float s, float g, float m) {
            const double e = ((double)s + bias) - (double)g;
            const double dr = eps2 > 0.0 ? e / sqrt(fma(e, e, eps2)) : e > 0.0 ? 1.0 : e < 0.0 ? -1.0 : e;    // e: 0, or NaN
            return (float)(coef * (double)m * (dr - sigma));
        };
    });
}

template <int PHASE>
void launch_walk(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, int ntx, int ntiles,
                 const double* nbias, double eps2, double* partial, hipStream_t stream) {
    with_border(border, [&](auto beta) {
        hipLaunchKernelGGL((cl1_walk_kernel<decltype(beta)::value, PHASE>), dim3(ntiles, B), dim3(256), 0, stream, srs, hrs, maps, H, W, clip,
                           ntx, nbias, eps2, partial);
    });
}

}  // namespace

// the tiles' sums (one buffer, used by the pre-pass and then by the main pass) and nbias
size_t hrn_cl1_loss_workspace_bytes_impl(int B, int H, int W, int border) {
    return (size_t)B * (tiles_of(H, W, border, nullptr) + 1) * nk_of(border) * 2 * sizeof(double);
}

int hrn_launch_cl1_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int clip, float eps,
                              float* out, double* stats, double* workspace, hipStream_t stream) {
    HRN_CHECK(border >= 0 && border <= OW_MAX_BORDER, -2, "cl1 loss: border %d outside 0..%d", border, OW_MAX_BORDER);
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
    hipLaunchKernelGGL(cl1_bias_kernel, dim3(B), dim3(OW_FIN_THREADS), 0, stream, (const double*)partial, ntiles, nk, nbias);
    HRN_LAUNCH_CHECK();
    if (eps == 0.f) launch_walk<CL_ABS>(srs, hrs, maps, B, H, W, border, clip, ntx, ntiles, nbias, 0.0, partial, stream);
    else launch_walk<CL_CHARB>(srs, hrs, maps, B, H, W, border, clip, ntx, ntiles, nbias, eps2, partial, stream);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl1_finish_kernel, dim3(B), dim3(OW_FIN_THREADS), 0, stream, (const double*)partial, (const double*)nbias, ntiles, nk,
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
