// The sub-pixel searched cMSE / cPSNR loss (the definition is in include/hrnet_hip.h, tests/subpixel_ref.py restates
// it in fp64): the prediction is registered to its target by the scene path's grid search, scored by the brightness-corrected cMSE instead
// of the NCC, and the gradient goes through the sampler at the point the search found.
//
// Forward.  m0 = (hr_map != 0) inside the border frame is written once into the workspace; then registration_scene.hip's means pre-pass
// and, per level, scene_level (mncc_scene.h) with V = 1, views = srs (no mask of their own), ref = hrs, ref_mask = m0: the six sums
// n, sum t, sum r, sum t^2, sum r^2, sum r t over c(s) = m0 and the footprint inside the frame, t = S(sr - mean sr, s), r = hr - mean hr
// under m0.  The finish of a level adds the tiles in index order and forms
//     cMSE = (sum t^2 + sum r^2 - 2 sum r t - (sum t - sum r)^2 / n) / n
// in fp64 - a constant subtracted from either image does not change it - takes the first maximum of -cMSE and leaves the next centre in
// device memory.  The last finish writes `out` and `stats`.  1 + 1 + 2 levels launches, nothing returns to the host, no atomics.
//
// Backward.  A tile kernel in scene_apply_kernel's shape forms t at s* with the forward's operations (the window of sr - mean, the row
// pass, the column run, the mean and the shift read back from `stats`), the residual e = t + bias - r in fp64 and writes g = factor e and
// c for its core into two workspace planes; resample_bwd.hip's d_views launch then applies the sampler's adjoint to them.  Two launches.
#include "mncc_scene.h"

namespace {

constexpr int SP_CPSNR = 2;                      // `metric` as hrn_get_loss has it: 1 = cMSE, 2 = cPSNR
constexpr int SP_STATS = 8;                      // n*, b*, cMSE*, dy*, dx*, mean sr, mean hr under m0, the centred bias
constexpr int SP_MASK_THREADS = 256, SP_MASK_BLOCKS = 4096;

// ----------------------------------------------------------------------------- m0
// m0 = 1 where the map is non-zero and the pixel is at least `border` from every frame edge, else 0.  A grid-stride loop over B H W.
__global__ __launch_bounds__(SP_MASK_THREADS) void subpixel_mask_kernel(const float* __restrict__ maps, int H, int W, int border, size_t hw,
                                                                        size_t total, float* __restrict__ m0) {
    const size_t step = (size_t)gridDim.x * SP_MASK_THREADS;
    for (size_t i = (size_t)blockIdx.x * SP_MASK_THREADS + threadIdx.x; i < total; i += step) {
        const size_t p = i % hw;
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        const bool in = y >= border && y < H - border && x >= border && x < W - border;
        m0[i] = in && maps[i] != 0.f ? 1.f : 0.f;
    }
}

// ----------------------------------------------------------------------------- one grid level: the tiles' sums
// scene_level_kernel's body with one view a sample: sums[((b * tiles + tile) * P^2 + i P + j) * 6 + q].  grid (B tiles)
__global__ __launch_bounds__(SC_THREADS) void subpixel_level_kernel(const float* __restrict__ hrs, const float* __restrict__ m0,
                                                                    const float* __restrict__ srs, const float* __restrict__ centres,
                                                                    const double* __restrict__ means, unsigned chunks, unsigned B, int H,
                                                                    int W, int P, double width, unsigned tiles_x, unsigned tiles,
                                                                    double* __restrict__ sums) {
    scene_level(hrs, m0, srs, nullptr, centres, means, chunks, B, 1, H, W, P, width, tiles_x, tiles, sums,
                [](size_t view, unsigned) { return view; });
}

// ----------------------------------------------------------------------------- one grid level: the finish
// the brightness-corrected cMSE out of the six sums s = {n, sum t, sum r, sum t^2, sum r^2, sum r t}, clamped at 0; n > 0
__device__ __forceinline__ double cmse_of_sums(const double* s) {
    const double n = s[0], d = s[1] - s[2];
    const double v = (((s[3] + s[4]) - 2.0 * s[5]) - d * d / n) / n;
    return v < 0.0 ? 0.0 : v;                    // a NaN stays a NaN
}

struct SubpixelFinish {
    double sums[SC_PMAX * SC_PMAX][RG_NSUM];
    double cmse[SC_PMAX * SC_PMAX];
    float coord[2][SC_PMAX];
};

// Per sample: the tiles' sums added in index order, the P^2 values of cMSE, the first maximum of -cMSE in row-major order (strict >, in
// fp64; a point without a counted pixel is -inf and a NaN is never taken) -> centres_out[b] = its point (the centre stays without one),
// trace_k[b * trace_stride] = (dy, dx, cMSE) (NaN without a point).  With `out` (the last level) also out[b] and stats[b].  centres_in
// null: (0, 0); centres_out may be centres_in.  grid (B), SC_FINISH_THREADS threads
__global__ __launch_bounds__(SC_FINISH_THREADS) void subpixel_finish_kernel(const double* __restrict__ sums, const float* centres_in, int P,
                                                                            double width, unsigned tiles, float* centres_out,
                                                                            float* __restrict__ trace_k, int trace_stride,
                                                                            const double* __restrict__ means, unsigned chunks, unsigned B,
                                                                            int metric, float* __restrict__ out, double* __restrict__ stats) {
    __shared__ SubpixelFinish F;
    const int tid = threadIdx.x, pp = P * P;
    const size_t b = blockIdx.x;
    float cy = centres_in ? centres_in[2 * b] : 0.f, cx = centres_in ? centres_in[2 * b + 1] : 0.f;
    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        F.coord[axis][i] = grid_coord((double)(axis ? cx : cy), width, i, P);
    }
    if (tid < pp) {
        double s[RG_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double* in = sums + (b * tiles * pp + tid) * RG_NSUM;
        for (unsigned t = 0; t < tiles; ++t, in += (size_t)pp * RG_NSUM)
#pragma unroll
            for (int q = 0; q < RG_NSUM; ++q) s[q] += in[q];
#pragma unroll
        for (int q = 0; q < RG_NSUM; ++q) F.sums[tid][q] = s[q];
        F.cmse[tid] = s[0] > 0.0 ? cmse_of_sums(s) : INFINITY;
    }
    __syncthreads();
    if (tid != 0) return;
    int at = -1;
    double best = -INFINITY;
    for (int i = 0; i < pp; ++i)
        if (F.sums[i][0] > 0.0 && -F.cmse[i] > best) { best = -F.cmse[i]; at = i; }
    if (at >= 0) { cy = F.coord[0][at / P]; cx = F.coord[1][at % P]; }
    const double cmse = at >= 0 ? F.cmse[at] : __longlong_as_double(0x7ff8000000000000LL);
    centres_out[2 * b] = cy;
    centres_out[2 * b + 1] = cx;
    if (trace_k) {
        float* tr = trace_k + b * trace_stride;
        tr[0] = cy; tr[1] = cx; tr[2] = (float)cmse;
    }
    if (!out) return;
    const float mean_sr = plane_mean(means, b, chunks), mean_hr = plane_mean(means, (size_t)B + b, chunks);
    double* st = stats + SP_STATS * b;
    st[3] = (double)cy; st[4] = (double)cx; st[5] = (double)mean_sr; st[6] = (double)mean_hr;
    if (at < 0) {                                // no counted pixel at any point: NaN, and the backward writes zeros
        st[0] = 0.0; st[1] = 0.0; st[2] = cmse; st[7] = 0.0;
        out[b] = __int_as_float(0x7fc00000);
        return;
    }
    const double* s = F.sums[at];
    const double bias = (s[2] - s[1]) / s[0];
    st[0] = s[0]; st[1] = bias + ((double)mean_hr - (double)mean_sr); st[2] = cmse; st[7] = bias;
    out[b] = metric == SP_CPSNR ? (float)(-10.0 * log10(cmse)) : (float)cmse;
}

// ----------------------------------------------------------------------------- the backward: g and c at s*
// For the core tile of one sample: t = S(sr - mean sr, s*) by the level kernel's operations in its order, r = hr - mean hr, c = m0 and
// the footprint inside the frame, e = (t + bias) - r in fp64 with the centred bias of `stats`, g = (float)(coef e) where c holds, else 0,
// coef = d_out[b] 2 / n* (times -10 / (ln 10 cMSE*) for cPSNR), 0 for a sample without a counted pixel.  g and c are resample_bwd.hip's
// d_out and valid; tile 0 also leaves s* as fp32 in shifts[b].  grid (B tiles)
__global__ __launch_bounds__(SC_THREADS) void subpixel_residual_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                                       const float* __restrict__ maps, const double* __restrict__ stats,
                                                                       const float* __restrict__ d_out, int H, int W, int border, int metric,
                                                                       unsigned tiles_x, unsigned tiles, float* __restrict__ g_out,
                                                                       float* __restrict__ c_out, float* __restrict__ shifts) {
    __shared__ SceneShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x / tiles, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)b * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;
    const double* st = stats + SP_STATS * b;
    if (tid < 2) {
        const float d = (float)st[3 + tid];
        split_and_taps(d, &S.whole[tid][0], &S.frac[tid][0], S.tap[tid][0]);
        if (tile == 0) shifts[2 * b + tid] = d;
    }
    __syncthreads();
    if (tid == 0) S.table[0] = mask_table(S.frac[0][0], S.frac[1][0]);
    const int ny = S.whole[0][0], nx = S.whole[1][0];
    constexpr int ROWS = SC_TILE + 5;
    stage_window<ROWS, ROWS>(srs + b * hw, nullptr, S, ty0 + ny - 2, tx0 + nx - 2, H, W, (float)st[5], tid);
    scene_row_pass(S, S.tap[1][0], 0, ROWS, tid);
    __syncthreads();
    const unsigned table = S.table[0];
    float ky[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][0][o];
    const double n = st[0], bias = st[7];
    const bool none = !(n > 0.0);
    double coef = none ? 0.0 : (double)d_out[b] * 2.0 / n;
    if (!none && metric == SP_CPSNR) coef *= -10.0 / (2.302585092994046 * st[2]);
    const float mean_hr = (float)st[6];
    const int x = lane, gx = tx0 + x;
    const bool xcrop = gx >= border && gx < W - border;
#pragma unroll
    for (int k = 0; k < SC_ITEMS; ++k) {
        const int yl = (wave + k * SC_WAVES) * RG_RUN, gy = ty0 + yl;
        float t[RG_RUN];
        const unsigned c = scene_column_run(S, ky, ny, nx, 0, 0, table, x, yl, gy, gx, H, W, t);
        if (gx >= W) continue;
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            const int y = gy + p;
            if (y >= H) break;
            const size_t i = b * hw + (size_t)y * W + gx;
            const bool on = !none && ((c >> p) & 1u) && xcrop && y >= border && y < H - border && maps[i] != 0.f;
            const float r = hrs[i] - mean_hr;
            const double e = ((double)t[p] + bias) - (double)r;
            g_out[i] = on ? (float)(coef * e) : 0.f;
            c_out[i] = on ? 1.f : 0.f;
        }
    }
}

// the parts of the workspace: the forward's m0 and the scene plan behind it; the backward's g, c and fp32 shifts
size_t plane_bytes(int B, int H, int W) { return (((size_t)B * H * W * sizeof(float)) + 15) & ~(size_t)15; }

}  // namespace

size_t hrn_subpixel_loss_forward_bytes_impl(int B, int H, int W, int P) { return plane_bytes(B, H, W) + plan(B, 1, H, W, P).bytes(); }

size_t hrn_subpixel_loss_backward_bytes_impl(int B, int H, int W) { return 2 * plane_bytes(B, H, W) + 8 * (size_t)B; }

int hrn_launch_subpixel_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int P, int levels,
                                   float radius, int metric, float* out, double* stats, float* trace, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, 1, H, W, P);
    float* m0 = static_cast<float*>(workspace);
    const SceneWorkspace w = carve(static_cast<unsigned char*>(workspace) + plane_bytes(B, H, W), p);
    const size_t hw = (size_t)H * W, total = (size_t)B * hw;
    HrnProfScope prof("subpixel_fwd", level_flops(P) * levels * B * H * W, 4.0 * B * (4.0 + 2.0 * levels) * H * W, stream);
    const size_t blocks = (total + SP_MASK_THREADS - 1) / SP_MASK_THREADS;
    hipLaunchKernelGGL(subpixel_mask_kernel, dim3((unsigned)(blocks < (size_t)SP_MASK_BLOCKS ? blocks : (size_t)SP_MASK_BLOCKS)),
                       dim3(SP_MASK_THREADS), 0, stream, maps, H, W, border, hw, total, m0);
    HRN_LAUNCH_CHECK();
    hrn_launch_mncc_scene_means(hrs, m0, srs, nullptr, B, 1, H, W, w.means, stream);
    HRN_LAUNCH_CHECK();
    double width = (double)(2.f * radius);
    const double ratio = level_ratio(P);
    for (int k = 0; k < levels; ++k) {
        const float* centres = k ? w.centres : nullptr;
        const bool last = k == levels - 1;
        hipLaunchKernelGGL(subpixel_level_kernel, dim3((unsigned)B * p.tiles), dim3(SC_THREADS), 0, stream, hrs, (const float*)m0, srs, centres,
                           (const double*)w.means, p.chunks, (unsigned)B, H, W, P, width, p.tiles_x, p.tiles, w.sums);
        HRN_LAUNCH_CHECK();
        hipLaunchKernelGGL(subpixel_finish_kernel, dim3(B), dim3(SC_FINISH_THREADS), 0, stream, (const double*)w.sums, centres, P, width,
                           p.tiles, w.centres, trace ? trace + 3 * k : (float*)nullptr, 3 * levels, (const double*)w.means, p.chunks,
                           (unsigned)B, metric, last ? out : (float*)nullptr, last ? stats : (double*)nullptr);
        HRN_LAUNCH_CHECK();
        width = width * ratio;
    }
    return 0;
}

int hrn_launch_subpixel_loss_backward(const float* srs, const float* hrs, const float* maps, const double* stats, const float* d_out, int B,
                                      int H, int W, int border, int metric, float* d_srs, void* workspace, hipStream_t stream) {
    const ScenePlan p = plan(B, 1, H, W, HRN_MNCC_MIN_POINTS);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    float* g = reinterpret_cast<float*>(base);
    float* c = reinterpret_cast<float*>(base + plane_bytes(B, H, W));
    float* shifts = reinterpret_cast<float*>(base + 2 * plane_bytes(B, H, W));
    HrnProfScope prof("subpixel_bwd", 2.0 * 24.0 * B * H * W, 32.0 * B * H * W, stream);
    hipLaunchKernelGGL(subpixel_residual_kernel, dim3((unsigned)B * p.tiles), dim3(SC_THREADS), 0, stream, srs, hrs, maps, stats, d_out, H, W,
                       border, metric, p.tiles_x, p.tiles, g, c, shifts);
    HRN_LAUNCH_CHECK();
    return hrn_launch_mncc_apply_backward(nullptr, shifts, c, g, B, 1, H, W, d_srs, nullptr, nullptr, stream);
}
