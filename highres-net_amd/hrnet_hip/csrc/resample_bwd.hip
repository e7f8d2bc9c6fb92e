// The backward of the six-tap sampler of the registration paths: out = S(view, shift) of hrn_mncc_apply_scene is
// linear in the view and C^1 in the shift, and these kernels give both gradients on the scene path's geometry - tiles of SC_TILE x
// SC_TILE, SC_THREADS threads, a lane per column, runs of RG_RUN rows.
//
// g = d_out where the pixel's `valid` is non-zero AND its 6 x 6 footprint lies inside the frame, else 0.  The kernels test the footprint
// themselves, so whatever `valid` holds nothing outside a frame is ever read.
//
// d_views(p, q) = sum_{a, b = -2..3} k^y_a k^x_b g(p - n_y - a, q - n_x - b), g zero outside the frame.  The shift is one per view, so
// the adjoint is a GATHER: the forward's two LDS passes with the taps reversed and the whole parts (-n_y - 1, -n_x - 1), with zero padding
// in place of the forward's "footprint leaves the frame => invalid".  One launch, a window of g (core + 5 rows and columns) staged once,
// every element of d_views written; no scatter, no atomic.
//
// d_shifts[., 0] = sum_pixels g dS/ddy, dS/ddy = the taps k'^y down the columns of the pass along rows with k^x; [., 1] the mirror.
// k'_o = (u'_o - k_o sum u') / sum u with u_o = L3(o - f), u'_o = -L3'(o - f), formed in fp64 per view and rounded to fp32 as
// split_and_taps rounds k.  One staged window of the view serves both derivative images: the pass along rows runs twice into the same
// buffer.  A pixel's product is fp32; a thread's sums, the wave's (WaveSums), the waves' and - in the finish launch - the tiles' in index
// order are fp64 in a fixed order, rounded to fp32 once.  Two launches.  A component of the shift at or beyond +-RG_DMAX (or a NaN) gets
// exactly 0: split_and_taps clamps it, and the clamp has zero slope.
//
// Both results are bit-reproducible and a view's does not depend on the batch around it.
#include "mncc_scene.h"

namespace {

constexpr int RB_WIN = SC_TILE + 5;             // window rows and columns: the core and the six-tap footprint at one offset
static_assert((SC_ITEMS * SC_WAVES - 1) * RG_RUN + RG_RUN + 5 == RB_WIN, "the last run's RG_RUN + 5 rows end with the window");

struct ResampleShared {
    float T[RB_WIN * RB_WIN];                   // the window: of g (d_views) or of the view (d_shifts)
    float A[RB_WIN * SC_TILE];                  // the pass along rows
    double red[SC_WAVES][2];
    double u[2][6], du[2][6];                   // L3(o - f) and its derivative in f per axis, axis 0 = y, before the normalisation
    float tap[2][6], dtap[2][6];                // k and k'
};
static_assert(sizeof(ResampleShared) <= 40 * 1024, "four workgroups per CU");

// Staging: a thread's RB_STAGE window pixels are loaded before the first is used.  A pixel that does not count reads element 0 of its
// plane - always inside the frame - and a select puts 0 in its place, so no load waits for a test and none leaves the frame.
constexpr int RB_STAGE = (RB_WIN * RB_WIN + SC_THREADS - 1) / SC_THREADS;
static_assert(RB_STAGE <= 32, "a thread's window pixels fit one 32-bit word of flags");

// sinc(t) = sin(pi t) / (pi t) and its derivative.  The closed form (cos(pi t) - sinc(t)) / t cancels near 0, so below 1e-2 the series
// pi (-z / 3 + z^3 / 30 - z^5 / 840), z = pi t, stands in: its first dropped term is below 3e-15 there.
__device__ void sinc_and_slope(double t, double* s, double* ds) {
    const double z = 3.141592653589793 * t;
    *s = t == 0.0 ? 1.0 : sin(z) / z;
    *ds = fabs(t) < 1e-2 ? 3.141592653589793 * z * (-1.0 / 3.0 + z * z * (1.0 / 30.0 - z * z / 840.0)) : (cos(z) - *s) / t;
}

// split_and_taps' split, for every thread: n = floor(d) and f = d - n of the clamped coordinate
__device__ __forceinline__ int whole_part(float d, double* f) {
    const float dc = fminf(fmaxf(d, -RG_DMAX), RG_DMAX);
    const double fl = floor((double)dc);
    *f = (double)dc - fl;
    return (int)fl;
}

// The taps of a view, a lane per tap instead of split_and_taps' one thread per axis - the fp64 sines are what a workgroup would wait
// for.  The operations on k are split_and_taps' in its order (u_o = sinc sinc, the six added from o = 0 up, the quotient rounded to
// fp32), and k'_o = (u'_o - k_o sum u') / sum u beside it.  tap_terms: lanes 0..11 of the workgroup, before a barrier; tap_finish:
// the same lanes after it, and another barrier before S.tap / S.dtap are read.
template <bool SLOPES>
__device__ __forceinline__ void tap_terms(ResampleShared& S, const double* f, int tid) {
    if (tid >= 12) return;
    const int axis = tid / 6, o = tid - axis * 6;
    const double x = (double)(o - 2) - f[axis];
    double a, da, b, db;
    sinc_and_slope(x, &a, &da);
    sinc_and_slope(x / 3.0, &b, &db);
    const bool out = fabs(x) >= 3.0;
    S.u[axis][o] = out ? 0.0 : a * b;
    if (SLOPES) S.du[axis][o] = out ? 0.0 : -(da * b + a * db / 3.0);     // u' = d/df L3(o - f) = -L3'(o - f)
}

template <bool SLOPES>
__device__ __forceinline__ void tap_finish(ResampleShared& S, int tid) {
    if (tid >= 12) return;
    const int axis = tid / 6, o = tid - axis * 6;
    double su = 0.0, sdu = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) { su += S.u[axis][j]; if (SLOPES) sdu += S.du[axis][j]; }
    S.tap[axis][o] = (float)(S.u[axis][o] / su);
    if (SLOPES) S.dtap[axis][o] = (float)((S.du[axis][o] - (S.u[axis][o] / su) * sdu) / su);
}

// is pixel y of an axis of length L inside it together with its footprint at the whole-pixel offset n
__device__ __forceinline__ bool footprint_inside(int y, int n, int L) { return y >= 0 && y < L && y + n - 2 >= 0 && y + n + 3 <= L - 1; }

// the pass along rows over the whole window: A[wy][x] = sum_m k[m] T[wy][x + m]; the last column read is 63 + 5 < RB_WIN
__device__ void window_row_pass(ResampleShared& S, const float* k, int tid) {
    const int x = tid & 63;
    for (int wy = tid >> 6; wy < RB_WIN; wy += SC_WAVES) {
        const float* row = S.T + wy * RB_WIN + x;
        float a = k[0] * row[0];
#pragma unroll
        for (int m = 1; m < 6; ++m) a = fmaf(k[m], row[m], a);
        S.A[wy * SC_TILE + x] = a;
    }
}

// the six taps down the RG_RUN + 5 rows of A under the run that begins in core row yl: the last row read is 56 + 12 < RB_WIN
__device__ __forceinline__ void window_column_run(const ResampleShared& S, const float* k, int x, int yl, float* t) {
    float a[RG_RUN + 5];
#pragma unroll
    for (int m = 0; m < RG_RUN + 5; ++m) a[m] = S.A[(yl + m) * SC_TILE + x];
    column_taps(k, a, t);
}

// ----------------------------------------------------------------------------- d_views
// grid (B V tiles); a workgroup writes the core tile (ty0, tx0) of d_views of one view
__global__ __launch_bounds__(SC_THREADS) void resample_bwd_views_kernel(const float* __restrict__ shifts, const float* __restrict__ valid,
                                                                        const float* __restrict__ d_out, int H, int W, unsigned tiles_x,
                                                                        unsigned tiles, float* __restrict__ d_views) {
    __shared__ ResampleShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;
    double f[2];
    const int ny = whole_part(shifts[2 * view], &f[0]), nx = whole_part(shifts[2 * view + 1], &f[1]);
    // the window of g: its pixel (0, 0) is the frame's (ty0 - n_y - 3, tx0 - n_x - 3), the forward's origin at the whole parts -n - 1
    {
        const float* go = d_out + view * hw;
        const float* va = valid + view * hw;
        const int oy = ty0 - ny - 3, ox = tx0 - nx - 3;
        float gv[RB_STAGE], vv[RB_STAGE];
        unsigned in = 0;
#pragma unroll
        for (int j = 0; j < RB_STAGE; ++j) {
            const int i = tid + j * SC_THREADS, wy = i / RB_WIN, wx = i - wy * RB_WIN;
            const int y = oy + wy, x = ox + wx;
            const bool ok = i < RB_WIN * RB_WIN && footprint_inside(y, ny, H) && footprint_inside(x, nx, W);
            const size_t g = ok ? (size_t)y * W + x : 0;
            vv[j] = va[g];
            gv[j] = go[g];
            in |= (unsigned)ok << j;
        }
        tap_terms<false>(S, f, tid);             // while the loads are under way
#pragma unroll
        for (int j = 0; j < RB_STAGE; ++j) {
            const int i = tid + j * SC_THREADS;
            if (i < RB_WIN * RB_WIN) S.T[i] = ((in >> j) & 1u) && vv[j] != 0.f ? gv[j] : 0.f;
        }
    }
    __syncthreads();
    tap_finish<false>(S, tid);
    __syncthreads();
    float kx[6], ky[6];                          // reversed: window column x + m holds g(q - n_x - a) for a = 3 - m, tap index 5 - m
#pragma unroll
    for (int m = 0; m < 6; ++m) { kx[m] = S.tap[1][5 - m]; ky[m] = S.tap[0][5 - m]; }
    window_row_pass(S, kx, tid);
    __syncthreads();
    const int x = lane, gx = tx0 + x;
    if (gx >= W) return;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const int yl = (wave + k * SC_WAVES) * RG_RUN, gy = ty0 + yl;
        float t[RG_RUN];
        window_column_run(S, ky, x, yl, t);
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            if (gy + p >= H) break;
            d_views[view * hw + (size_t)(gy + p) * W + gx] = t[p];
        }
    }
}

// ----------------------------------------------------------------------------- d_shifts: the tiles' sums
// partial[(view * tiles + tile) * 2 + axis] = sum over the tile's pixels of g dS/dd_axis.  grid (B V tiles)
__global__ __launch_bounds__(SC_THREADS) void resample_bwd_shifts_kernel(const float* __restrict__ views, const float* __restrict__ shifts,
                                                                         const float* __restrict__ valid, const float* __restrict__ d_out,
                                                                         int H, int W, unsigned tiles_x, unsigned tiles,
                                                                         double* __restrict__ partial) {
    __shared__ ResampleShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;
    double f[2];
    const int ny = whole_part(shifts[2 * view], &f[0]), nx = whole_part(shifts[2 * view + 1], &f[1]);
    // the window of the view as the forward stages it: its pixel (0, 0) is the frame's (ty0 + n_y - 2, tx0 + n_x - 2), zeros outside
    float tv[RB_STAGE];
    unsigned have = 0;
    {
        const float* vp = views + view * hw;
        const int oy = ty0 + ny - 2, ox = tx0 + nx - 2;
#pragma unroll
        for (int j = 0; j < RB_STAGE; ++j) {
            const int i = tid + j * SC_THREADS, wy = i / RB_WIN, wx = i - wy * RB_WIN;
            const int y = oy + wy, wxf = ox + wx;
            const bool ok = i < RB_WIN * RB_WIN && y >= 0 && y < H && wxf >= 0 && wxf < W;
            tv[j] = vp[ok ? (size_t)y * W + wxf : 0];
            have |= (unsigned)ok << j;
        }
    }
    // this thread's g, and which of its pixels count
    const int x = lane, gx = tx0 + x;
    float g[SC_ITEMS][RG_RUN];
    unsigned on = 0;
    {
        const float* go = d_out + view * hw;
        const float* va = valid + view * hw;
        const bool xin = footprint_inside(gx, nx, W);
#pragma unroll
        for (int k = 0; k < SC_ITEMS; ++k)
#pragma unroll
            for (int p = 0; p < RG_RUN; ++p) {
                const int gy = ty0 + (wave + k * SC_WAVES) * RG_RUN + p;
                const bool in = xin && footprint_inside(gy, ny, H);
                const size_t i = in ? (size_t)gy * W + gx : 0;
                const float v = va[i], d = go[i];
                const bool m = in && v != 0.f;
                g[k][p] = m ? d : 0.f;
                on |= (unsigned)m << (RG_RUN * k + p);
            }
    }
    tap_terms<true>(S, f, tid);                  // while the loads are under way
#pragma unroll
    for (int j = 0; j < RB_STAGE; ++j) {
        const int i = tid + j * SC_THREADS;
        if (i < RB_WIN * RB_WIN) S.T[i] = (have >> j) & 1u ? tv[j] : 0.f;
    }
    __syncthreads();
    tap_finish<true>(S, tid);
    __syncthreads();
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int axis = 0; axis < 2; ++axis) {       // axis 0: d/ddy = k^x along rows, k'^y down columns; axis 1: k'^x, k^y
        float kx[6], ky[6];
#pragma unroll
        for (int o = 0; o < 6; ++o) { kx[o] = axis ? S.dtap[1][o] : S.tap[1][o]; ky[o] = axis ? S.tap[0][o] : S.dtap[0][o]; }
        window_row_pass(S, kx, tid);
        __syncthreads();
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < SC_ITEMS; ++k) {
            float t[RG_RUN];
            window_column_run(S, ky, x, (wave + k * SC_WAVES) * RG_RUN, t);
#pragma unroll
            for (int p = 0; p < RG_RUN; ++p) {
                const float prod = (on >> (RG_RUN * k + p)) & 1u ? g[k][p] * t[p] : 0.f;
                s += (double)prod;
            }
        }
        sum[axis] = s;
        __syncthreads();                         // A is free again after this
    }
    WaveSums<2, 0>::run(sum, lane);
    if (lane < 2) S.red[wave][wave_sums_index<2>(lane)] = sum[0];
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int w = 0; w < SC_WAVES; ++w) s += S.red[w][tid];
        partial[(size_t)blockIdx.x * 2 + tid] = s;
    }
}

// ----------------------------------------------------------------------------- d_shifts: the finish
// d_shifts[view][axis] = the tiles' sums added in index order, rounded to fp32; exactly 0 where the coordinate is at or beyond the clamp
// of split_and_taps, or a NaN.  A thread per (view, axis)
constexpr int RB_FINISH_THREADS = 256;
__global__ __launch_bounds__(RB_FINISH_THREADS) void resample_bwd_finish_kernel(const double* __restrict__ partial,
                                                                               const float* __restrict__ shifts, size_t n, unsigned tiles,
                                                                               float* __restrict__ d_shifts) {
    const size_t i = (size_t)blockIdx.x * RB_FINISH_THREADS + threadIdx.x;       // 2 view + axis
    if (i >= n) return;
    const double* in = partial + (i >> 1) * tiles * 2 + (i & 1);
    double s = 0.0;
    for (unsigned t = 0; t < tiles; ++t) s += in[(size_t)t * 2];
    d_shifts[i] = fabsf(shifts[i]) < RG_DMAX ? (float)s : 0.f;
}

}  // namespace

size_t hrn_mncc_apply_backward_workspace_bytes_impl(int B, int V, int H, int W) {
    return 16 * (size_t)B * V * plan(B, V, H, W, HRN_MNCC_MIN_POINTS).tiles;
}

// d_views or d_shifts may be null: that half is not launched.  views and workspace are read only for d_shifts.
int hrn_launch_mncc_apply_backward(const float* views, const float* shifts, const float* valid, const float* d_out, int B, int V, int H,
                                   int W, float* d_views, float* d_shifts, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, V, H, W, HRN_MNCC_MIN_POINTS);
    const unsigned bv = (unsigned)(B * V);
    const double pixels = (double)B * V * H * W;
    if (d_views) {
        HrnProfScope prof("mncc_apply_backward_views", 2.0 * 12.0 * pixels, 12.0 * pixels, stream);
        hipLaunchKernelGGL(resample_bwd_views_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, shifts, valid, d_out, H, W, p.tiles_x,
                           p.tiles, d_views);
        HRN_LAUNCH_CHECK();
    }
    if (d_shifts) {
        HrnProfScope prof("mncc_apply_backward_shifts", 2.0 * 26.0 * pixels, 12.0 * pixels, stream);
        double* partial = static_cast<double*>(workspace);
        hipLaunchKernelGGL(resample_bwd_shifts_kernel, dim3(bv * p.tiles), dim3(SC_THREADS), 0, stream, views, shifts, valid, d_out, H, W,
                           p.tiles_x, p.tiles, partial);
        HRN_LAUNCH_CHECK();
        const size_t n = 2 * (size_t)bv;
        hipLaunchKernelGGL(resample_bwd_finish_kernel, dim3((unsigned)((n + RB_FINISH_THREADS - 1) / RB_FINISH_THREADS)), dim3(RB_FINISH_THREADS),
                           0, stream, (const double*)partial, shifts, n, p.tiles, d_shifts);
        HRN_LAUNCH_CHECK();
    }
    return 0;
}
