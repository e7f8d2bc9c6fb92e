// The shift-searched cMSE / cPSNR as a differentiable training tail:
//   shift_cPSNR(sr, hr, hr_map, border_w)   reference src/Evaluator.py:52-73   (the search over the integer offsets of hr)
//   get_loss(srs, hrs, hr_maps, metric)     reference src/train.py:66-87       (the per-offset brightness-corrected cMSE)
// With beta = border, h = H - 2 beta, w = W - 2 beta, s = the centre crop of sr, and for the offset k = u (2 beta + 1) + v
//   g = hr[u:u+h, v:v+w], m = map[u:u+h, v:v+w], d = s - g, S0 = sum m, S1 = sum m d, S2 = sum m d^2:
//   n_k = S0, bias_k = -S1 / S0, cMSE_k = (S2 - S1^2 / S0) / S0        (one pass, three fp64 sums: losses.hip)
// and k* = the lowest k of minimal cMSE_k among the offsets with n_k > 0.  The gradient goes through k* alone:
//   d out / d sr[beta + y, beta + x] = c m*[y, x] (s[y, x] + bias* - g*[y, x]),  c = 2 / n*  or  -20 / (ln 10 n* cMSE*)
//
// Forward, stage 1: offset_walk.h's walk of a 32 x 128 tile over the (2 beta + 1)^2 offsets, with the three sums of the square as its
// term.  Every pixel of the three images comes from HBM once (the halo re-reads of neighbouring tiles hit L2): 12 B H W bytes.  Stage 2
// adds the tiles' sums in a fixed order (runs of tiles in parallel, the runs in order) and picks k*.  No floating-point atomics: the
// result is bit-reproducible.
#include "offset_walk.h"

namespace {

// {S0, S1, S2} of d = s - g under the map
struct SquareTerm {
    static constexpr int SUMS = 3;
    struct Row {};
    template <int NB>
    __device__ __forceinline__ Row row(int) const { return Row(); }
    __device__ __forceinline__ void add(Row, int, double mm, double sd, double gd, double* a) const {
        const double d = sd - gd;
        const double md = mm * d;
        a[0] += mm;
        a[1] += md;
        a[2] = fma(md, d, a[2]);
    }
};

// grid (tiles, B).  partial [B][tiles][(2 beta + 1)^2][3] = {S0, S1, S2} of the tile at every offset.
template <int BETA>
__global__ __launch_bounds__(256) void shift_loss_partial_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                                 const float* __restrict__ maps, int H, int W, int clip, int ntx,
                                                                 double* __restrict__ partial) {
    offset_walk<BETA>(srs, hrs, maps, H, W, clip, ntx, SquareTerm(), partial);
}

// grid (B), 1024 threads.  Adds the tiles in a fixed order, then takes the lowest k of minimal cMSE_k among n_k > 0.
__global__ __launch_bounds__(OW_FIN_THREADS) void shift_loss_finish_kernel(const double* __restrict__ partial, int ntiles, int nk, int metric,
                                                                           float* __restrict__ out, double* __restrict__ stats) {
    __shared__ double acc[OW_FIN_THREADS];
    __shared__ double cn[OW_MAXK], cb[OW_MAXK], cm[OW_MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nv = 3 * nk;                               // <= 867
    const int runs = sum_tile_runs(partial + (size_t)b * ntiles * nv, ntiles, nv, acc);
    __syncthreads();
    for (int k = tid; k < nk; k += OW_FIN_THREADS) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < runs; ++r) {
            const double* o = acc + r * nv + 3 * k;
            s0 += o[0]; s1 += o[1]; s2 += o[2];
        }
        cn[k] = s0; cb[k] = -s1 / s0; cm[k] = (s2 - s1 * s1 / s0) / s0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best = -1;
    for (int k = 0; k < nk; ++k)
        if (cn[k] > 0.0 && (best < 0 || cm[k] < cm[best])) best = k;
    double* st = stats + 4 * (size_t)b;
    if (best < 0) {                                      // no clear pixel at any offset: NaN, and the backward writes zeros
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        st[0] = 0.0; st[1] = 0.0; st[2] = nan; st[3] = -1.0;
        out[b] = __int_as_float(0x7fc00000);
        return;
    }
    st[0] = cn[best]; st[1] = cb[best]; st[2] = cm[best]; st[3] = (double)best;
    out[b] = metric == 1 ? (float)cm[best] : (float)(-10.0 * log10(cm[best]));
}

// grid (rows of blocks, B): offset_walk.h's backward pass, the gradient in fp32.
__global__ __launch_bounds__(256) void shift_loss_backward_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                                  const float* __restrict__ maps, const double* __restrict__ stats,
                                                                  const float* __restrict__ d_out, int H, int W, int border, int metric,
                                                                  int clip, float* __restrict__ d_srs) {
    offset_walk_backward<4>(srs, hrs, maps, stats, H, W, border, clip, d_srs, [=](const double* st, bool none) {
        const double cnt = st[0], cmse = st[2];
        // d out / d cMSE: cMSE itself -> 1;  -10 log10(cMSE) -> -10 / (ln 10 cMSE)
        const double dm = metric == 1 ? 1.0 : -10.0 / (2.302585092994046 * cmse);
        const float coef = none ? 0.f : (float)((double)d_out[blockIdx.y] * dm * 2.0 / cnt);
        const float fb = (float)st[1];
        return [=](float s, float g, float m) { return coef * m * (s - g + fb); };
    });
}

}  // namespace

size_t hrn_shift_loss_workspace_bytes_impl(int B, int H, int W, int border) {
    return (size_t)B * tiles_of(H, W, border, nullptr) * nk_of(border) * 3 * sizeof(double);
}

int hrn_launch_shift_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int metric,
                                int clip, float* out, double* stats, double* partial, hipStream_t stream) {
    HRN_CHECK(border >= 0 && border <= OW_MAX_BORDER, -2, "shift loss: border %d outside 0..%d", border, OW_MAX_BORDER);
    int ntx = 0;
    const size_t tiles = tiles_of(H, W, border, &ntx);
    HRN_CHECK(tiles <= 0x7fffffffu, -2, "shift loss: %zu tiles exceed the grid limit", tiles);
    const int ntiles = (int)tiles, nk = (int)nk_of(border);
    HrnProfScope prof("shift_loss_fwd", 0.0, 12.0 * B * H * W, stream);
    with_border(border, [&](auto beta) {
        hipLaunchKernelGGL(shift_loss_partial_kernel<decltype(beta)::value>, dim3(ntiles, B), dim3(256), 0, stream, srs, hrs, maps, H, W, clip,
                           ntx, partial);
    });
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(shift_loss_finish_kernel, dim3(B), dim3(OW_FIN_THREADS), 0, stream, (const double*)partial, ntiles, nk, metric, out, stats);
    HRN_LAUNCH_CHECK();
    return 0;
}

int hrn_launch_shift_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                   int H, int W, int border, int metric, int clip, float* d_srs, hipStream_t stream) {
    HrnProfScope prof("shift_loss_bwd", 0.0, 16.0 * B * H * W, stream);
    size_t gx = ((size_t)H * W + 1023) / 1024;          // four pixels per thread
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(shift_loss_backward_kernel, dim3((unsigned)gx, B), dim3(256), 0, stream, srs, hrs, maps, stats, d_out, H, W, border,
                       metric, clip, d_srs);
    HRN_LAUNCH_CHECK();
    return 0;
}
