// Shift-and-add (normalised convolution): every clear LR sample of every registered view placed at its sub-pixel position on the x2 / x3 /
// x4 grid, each HR pixel the weighted mean of the samples near it, and the adjoint (hrn_shift_add / hrn_shift_add_backward; the definition
// is in include/hrnet_hip.h).  (No counterpart in the reference, which has no classical multi-frame predictor.)
//
// Along an axis, HR index Y = S m + p of a view shifted by dy reads the view rows m + n_p - 1 .. m + n_p + 2, n_p = floor(d_p),
// d_p = t_p + dy.  t_p grows by less than 1 over the phases, so n_p is n_0 or n_0 + 1: every phase reads among the FIVE rows
// m + n_0 - 1 .. m + n_0 + 3, and its four weights are stored five wide, w5[p][e_p + k] = k(k - 1 - f_p), e_p = n_p - n_0, the fifth 0.
// No tap index depends on a run-time value after that: no array is indexed by one, no select, no scratch.  The weights are formed in fp64
// by the kernels themselves (the shifts live on the device), one (view, axis, phase, slot) per thread, and kept in LDS.
//
// Forward: a workgroup of 256 threads owns TH x TW = 8 x 32 LR cells of one sample (S TH x S TW output pixels) and walks the views in
// index order, in chunks of kChunk whose weights it forms first.  A view that does not count (alpha 0, a non-finite shift) is skipped - the
// branch is uniform; the chunk's counting views are compacted into a list first.  (The tile, its walk, the test of a view and the list
// are lr_tile.h's, shared with upsample.hip and observe.hip.)  Per view:
//   1. rawx / rawm[TH + 4][TW + 4]  <- m x and m of the window whose origin is moved by (n_0y, n_0x); the mask, the frame test at the load
//      (a thread's loads issued together, and the NEXT view's in flight during passes 2 and 3)
//   2. hx / hm[TH + 4][S TW]        <- the column taps of both planes (five fmas per phase, slots ascending)
//   3. a thread holds N, D of one LR row x four output columns x S phases in registers and adds the row taps of hx / hm to them:
//      five 16-byte LDS reads per plane, five fmas per phase and element, slots ascending, views in order
// then out = (N + prior b) / (D + prior) with the fallback, 16-byte stores where the row allows (chosen per row, as in upsample.hip); base
// is read by the thread that writes the same elements, so base == out is in place.
//
// Backward, d_views: a workgroup owns 8 x 32 pixels of ONE view and gathers.  View row i receives from cell m = i - n_0 + 1 - j, phase p,
// with w5[p][j], j = 0 .. 4: the cells i - n_0 - 3 .. i - n_0 + 1.
//   1. qs[(TH + 4) S][(TW + 4) S]  <- q = d_out / (weight + prior) (0 under the threshold) of those cells, zero outside the grid
//   2. tv[TH][(TW + 4) S]          <- the row gather of every staged column (j descending = cells ascending, phases ascending)
//   3. d_views                     <- the column gather of tv, times [clear]
// d_base is one element-wise kernel.  Neither kernel uses atomics; each element has one writer and one fixed order.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are stated in DESIGN.md section 7s.
#include "lr_tile.h"

#include <cmath>

namespace {

constexpr int kChunk = 32;                               // views whose weights a workgroup forms at a time
static_assert(kChunk <= 64, "compact_chunk takes a chunk in one wave");
constexpr float kMinDen = 9.5367431640625e-07f;          // 2^-20
constexpr float kMaxShift = 256.f;
constexpr double kMinTap = 8.673617379884035e-19;        // 2^-60: a smaller tap weight is taken as 0

// d_p of a shift component: fp64 sum, rounded to fp32, clamped to +-256
__device__ __forceinline__ float tap_coord(int S, int p, float shift) {
    const float d = (float)(((double)p + 0.5) / (double)S - 0.5 + (double)shift);
    return fminf(fmaxf(d, -kMaxShift), kMaxShift);
}

// k(u) = exp(-u^2 / (2 sigma^2)) cos^2(pi u / 4) inside |u| < 2, fp64
__device__ __forceinline__ double tap_kernel(double u, double sigma) {
    if (!(fabs(u) < 2.0)) return 0.0;
    const double c = cos(M_PI * u / 4.0);
    return exp(-(u * u) / (2.0 * sigma * sigma)) * c * c;
}

// slot j (0 .. 4) of phase p of an axis shifted by `shift`: the weight of view index m + n_0 - 1 + j
__device__ __forceinline__ float slot_weight(int S, int p, int j, float shift, float sigma) {
    const float d0 = tap_coord(S, 0, shift), d = tap_coord(S, p, shift);
    const float n = floorf(d);
    const int k = j - (int)(n - floorf(d0));             // tap o = k - 1
    if (k < 0 || k > 3) return 0.f;
    const double w = tap_kernel((double)(k - 1) - ((double)d - (double)n), (double)sigma);
    return w < kMinTap ? 0.f : (float)w;                 // every product k_y k_x that is kept is a normal fp32 number
}

// five slots ascending: w0 f0, then one fma per further slot
__device__ __forceinline__ float slots5(const float* w, float f0, float f1, float f2, float f3, float f4) {
    return fmaf(w[4], f4, fmaf(w[3], f3, fmaf(w[2], f2, fmaf(w[1], f1, w[0] * f0))));
}

// base and out may be the same pointer (no __restrict__ on either)
template <int S>
__global__ __launch_bounds__(kThreads) void shift_add_kernel(const float* __restrict__ views, const float* __restrict__ masks,
                                                             const float* __restrict__ alphas, const float* __restrict__ shifts,
                                                             const float* base, float* out, float* __restrict__ weight, size_t tiles, int V,
                                                             int H, int W, unsigned tiles_x, unsigned tiles_y, float sigma, float prior) {
    constexpr int RH = kTH + 4, RW = kTW + 4, HW_ = S * kTW, VPR = HW_ / 4;
    static_assert(kTH * VPR <= kThreads, "a thread holds the accumulators of one LR row x four output columns");
    __shared__ float rawx[RH][RW], rawm[RH][RW];
    __shared__ __attribute__((aligned(16))) float hx[RH][HW_], hm[RH][HW_];
    __shared__ float w5[kChunk][2][S][5];                // [view of the chunk][axis: 0 rows, 1 columns][phase][slot]
    __shared__ int n0[kChunk][2];                        // floor(d_0) per axis
    __shared__ int list[kChunk], n_list;                 // the views of the chunk that count, in index order
    constexpr int LPT = (RH * RW + kThreads - 1) / kThreads;            // window elements a thread stages
    const int SH = S * H, SW = S * W, tid = threadIdx.x;
    const int y = tid / VPR, c4 = tid - y * VPR;         // this thread's LR row of the tile and group of four output columns
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);
        f32x4 N[S], D[S];
#pragma unroll
        for (int p = 0; p < S; ++p) N[p] = D[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int v0 = 0; v0 < V; v0 += kChunk) {
            const int nv = min(kChunk, V - v0);
            __syncthreads();                             // the previous chunk's (or tile's) last reads of w5 / n0 / list are done
            for (int e = tid; e < nv * 2 * S * 5; e += kThreads) {
                const int j = e % 5, p = (e / 5) % S, ax = (e / (5 * S)) % 2, vi = e / (10 * S);
                const size_t bv = tp.n * (size_t)V + (size_t)(v0 + vi);
                const float sh = view_counts(alphas, shifts, bv) ? shifts[2 * bv + ax] : 0.f;
                w5[vi][ax][p][j] = slot_weight(S, p, j, sh, sigma);
                if (p == 0 && j == 0) n0[vi][ax] = (int)floorf(tap_coord(S, 0, sh));
            }
            if (tid < 64)                                // the first wave compacts the chunk's counting views (kChunk <= 64)
                compact_chunk(tid < nv && view_counts(alphas, shifts, tp.n * (size_t)V + (size_t)(v0 + min(tid, nv - 1))), list, &n_list);
            __syncthreads();
            // The window of a view: tile + 4 rows / columns from (y0 + n_0y - 1, x0 + n_0x - 1).  A thread's LPT elements are loaded
            // together - value and mask unconditionally wherever the element is inside the frame, so no load waits for another - and
            // the NEXT view's are in flight while this view's two passes run.
            float px[LPT], pm[LPT];
            auto fetch = [&](int vi) {
                const size_t plane = (tp.n * (size_t)V + (size_t)(v0 + vi)) * (size_t)H * W;
                const int wy0 = tp.y0 + n0[vi][0] - 1, wx0 = tp.x0 + n0[vi][1] - 1;
#pragma unroll
                for (int i = 0; i < LPT; ++i) {
                    const int e = tid + i * kThreads, r = e / RW, c = e - r * RW;
                    const int gy = wy0 + r, gx = wx0 + c;
                    const bool in = e < RH * RW && gy >= 0 && gy < H && gx >= 0 && gx < W;
                    const size_t at = plane + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
                    px[i] = in ? views[at] : 0.f;
                    pm[i] = in ? (masks ? masks[at] : 1.f) : 0.f;
                }
            };
            const int nl = n_list;
            if (nl > 0) fetch(list[0]);
            for (int li = 0; li < nl; ++li) {
                const int vi = list[li];
#pragma unroll
                for (int i = 0; i < LPT; ++i) {
                    const int e = tid + i * kThreads, r = e / RW, c = e - r * RW;
                    if (e < RH * RW) {
                        const bool clear = pm[i] != 0.f;
                        rawx[r][c] = clear ? px[i] : 0.f;
                        rawm[r][c] = clear ? 1.f : 0.f;
                    }
                }
                __syncthreads();                         // also: every thread is past the previous view's reads of hx / hm
                if (li + 1 < nl) fetch(list[li + 1]);
                for (int e = tid; e < RH * kTW; e += kThreads) {
                    const int r = e / kTW, x = e - r * kTW;
                    float fx[5], fm[5];
#pragma unroll
                    for (int k = 0; k < 5; ++k) { fx[k] = rawx[r][x + k]; fm[k] = rawm[r][x + k]; }
#pragma unroll
                    for (int p = 0; p < S; ++p) {
                        const float* w = w5[vi][1][p];
                        hx[r][S * x + p] = slots5(w, fx[0], fx[1], fx[2], fx[3], fx[4]);
                        hm[r][S * x + p] = slots5(w, fm[0], fm[1], fm[2], fm[3], fm[4]);
                    }
                }
                __syncthreads();                         // also: the next view's raw is not written before this
                if (tid < kTH * VPR) {
                    f32x4 a[5], b[5];
#pragma unroll
                    for (int k = 0; k < 5; ++k) { a[k] = *(const f32x4*)&hx[y + k][4 * c4]; b[k] = *(const f32x4*)&hm[y + k][4 * c4]; }
#pragma unroll
                    for (int p = 0; p < S; ++p) {
                        const float* w = w5[vi][0][p];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            N[p][k] += slots5(w, a[0][k], a[1][k], a[2][k], a[3][k], a[4][k]);
                            D[p][k] += slots5(w, b[0][k], b[1][k], b[2][k], b[3][k], b[4][k]);
                        }
                    }
                }
            }
        }
        const int ox = S * tp.x0 + 4 * c4;
        if (tid < kTH * VPR && tp.y0 + y < H && ox < SW) {
#pragma unroll
            for (int p = 0; p < S; ++p) {
                const size_t row = (tp.n * (size_t)SH + (size_t)(S * (tp.y0 + y) + p)) * (size_t)SW;
                float* orow = out + row;
                float* wrow = weight ? weight + row : nullptr;
                const float* brow = base ? base + row : nullptr;
                const bool vec = ox + 4 <= SW && ((uintptr_t)orow & 15u) == 0 && ((uintptr_t)brow & 15u) == 0 && ((uintptr_t)wrow & 15u) == 0;
                f32x4 b = {0.f, 0.f, 0.f, 0.f}, o;
                if (brow) {
                    if (vec) b = *(const f32x4*)(brow + ox);
                    else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (ox + k < SW) b[k] = brow[ox + k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float den = D[p][k] + prior;
                    o[k] = den >= kMinDen ? fmaf(prior, b[k], N[p][k]) / den : b[k];
                }
                if (vec) {
                    *(f32x4*)(orow + ox) = o;
                    if (wrow) *(f32x4*)(wrow + ox) = D[p];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ox + k < SW) {
                            orow[ox + k] = o[k];
                            if (wrow) wrow[ox + k] = D[p][k];
                        }
                }
            }
        }
    }
}

template <int S>
__global__ __launch_bounds__(kThreads) void shift_add_bwd_views_kernel(const float* __restrict__ d_out, const float* __restrict__ weight,
                                                                       const float* __restrict__ masks, const float* __restrict__ alphas,
                                                                       const float* __restrict__ shifts, float* __restrict__ d_views,
                                                                       size_t tiles, int V, int H, int W, unsigned tiles_x, unsigned tiles_y,
                                                                       float sigma, float prior) {
    constexpr int CY = kTH + 4, CX = kTW + 4, GR = CY * S, GC = CX * S;
    __shared__ float qs[GR][GC];
    __shared__ float tv[kTH][GC];
    __shared__ float w5[2][S][5];
    const int SH = S * H, SW = S * W, tid = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);        // tp.n: the view's plane, b V + v
        const int ty = tid / kTW, tx = tid - ty * kTW;              // kThreads == kTH * kTW
        const bool inside = tp.y0 + ty < H && tp.x0 + tx < W;
        const size_t at = tp.n * (size_t)H * W + (size_t)(tp.y0 + ty) * W + (tp.x0 + tx);
        if (!view_counts(alphas, shifts, tp.n)) {                   // uniform
            if (inside) d_views[at] = 0.f;
            continue;
        }
        const float dy = shifts[2 * tp.n], dx = shifts[2 * tp.n + 1];
        if (tid < 2 * S * 5) {
            const int j = tid % 5, p = (tid / 5) % S, ax = tid / (5 * S);
            w5[ax][p][j] = slot_weight(S, p, j, ax ? dx : dy, sigma);
        }
        // the first staged cell: rows i - n_0 - 3 .. i - n_0 + 1 of i = y0 .. y0 + TH - 1
        const int cy0 = tp.y0 - (int)floorf(tap_coord(S, 0, dy)) - 3, cx0 = tp.x0 - (int)floorf(tap_coord(S, 0, dx)) - 3;
        const size_t b = tp.n / (size_t)V;
        const float* g = d_out + b * (size_t)SH * SW;
        const float* wt = weight + b * (size_t)SH * SW;
        // four elements of a thread at a time, their loads of d_out and weight issued together (neither waits for the other)
        for (int e0 = tid; e0 < GR * GC; e0 += 4 * kThreads) {
            float gv[4], wv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * kThreads, r = e / GC, c = e - r * GC;
                const long oy = (long)S * cy0 + r, ox = (long)S * cx0 + c;
                const bool in = e < GR * GC && oy >= 0 && oy < SH && ox >= 0 && ox < SW;
                const size_t o = in ? (size_t)oy * SW + (size_t)ox : 0;
                gv[i] = in ? g[o] : 0.f;
                wv[i] = in ? wt[o] : -1.f;                           // outside the grid: under the threshold, q = 0
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * kThreads, r = e / GC, c = e - r * GC;
                const float den = wv[i] + prior;
                if (e < GR * GC) qs[r][c] = wv[i] >= 0.f && den >= kMinDen ? gv[i] / den : 0.f;
            }
        }
        __syncthreads();
        for (int e = tid; e < kTH * GC; e += kThreads) {
            const int yy = e / GC, c = e - yy * GC;
            float acc = 0.f;
#pragma unroll
            for (int j = 4; j >= 0; --j)                            // cell (yy + 4 - j) of the staged ones: i - n_0 + 1 - j
#pragma unroll
                for (int p = 0; p < S; ++p) acc = fmaf(w5[0][p][j], qs[(yy + 4 - j) * S + p][c], acc);
            tv[yy][c] = acc;
        }
        __syncthreads();
        if (inside) {
            float acc = 0.f;
#pragma unroll
            for (int j = 4; j >= 0; --j)
#pragma unroll
                for (int p = 0; p < S; ++p) acc = fmaf(w5[1][p][j], tv[ty][(tx + 4 - j) * S + p], acc);
            d_views[at] = (!masks || masks[at] != 0.f) ? acc : 0.f;
        }
        __syncthreads();                                            // qs, tv and w5 are free for the next tile
    }
}

// d_base = prior q, or d_out where the fallback holds
__global__ __launch_bounds__(kThreads) void shift_add_bwd_base_kernel(const float* __restrict__ d_out, const float* __restrict__ weight,
                                                                      float* __restrict__ d_base, size_t n, float prior) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const float den = weight[i] + prior, g = d_out[i];
        d_base[i] = den >= kMinDen ? prior * (g / den) : g;
    }
}

// what both entry points refuse; -> true, or false with the error set
bool check_shape(const char* fn, int B, int V, int H, int W, int scale, float sigma, float prior, unsigned* tiles_x, unsigned* tiles_y) {
    *tiles_x = *tiles_y = 0;
    if (!(B > 0 && V > 0 && H > 0 && W > 0)) { hrn_set_error("%s: empty input B=%d V=%d H=%d W=%d", fn, B, V, H, W); return false; }
    if (!check_side_scale(fn, "frames", H, W, scale)) return false;
    if (!(std::isfinite(sigma) && sigma >= 0.1f && sigma <= 1.f)) { hrn_set_error("%s: sigma must lie in [0.1, 1] (got %g)", fn, (double)sigma); return false; }
    if (!(std::isfinite(prior) && prior >= 0.f)) { hrn_set_error("%s: prior must be finite and >= 0 (got %g)", fn, (double)prior); return false; }
    // 2^62 elements (upsample.hip's limit too; observe.hip stops at 2^60; no reason for the difference is recorded)
    if ((size_t)B > ((size_t)1 << 62) / ((size_t)V * scale * scale * H * W)) {
        hrn_set_error("%s: %d x %d frames of %d x %d exceed the address space", fn, B, V, H, W);
        return false;
    }
    plane_tiles(H, W, tiles_x, tiles_y);
    return true;
}

}  // namespace

extern "C" int hrn_shift_add(const float* views, const float* view_masks, const float* alphas, const float* shifts, const float* base,
                             float* out, float* weight, int B, int V, int H, int W, int scale, float sigma, float prior, void* stream_) {
    HRN_CHECK(views && shifts && out, -2, "hrn_shift_add: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_shift_add", B, V, H, W, scale, sigma, prior, &tx, &ty)) return -2;
    const size_t lr = (size_t)B * V * H * W, sr = (size_t)B * H * W * scale * scale, lrb = lr * sizeof(float), srb = sr * sizeof(float);
    HRN_CHECK(!overlaps(views, lrb, out, srb) && !(view_masks && overlaps(view_masks, lrb, out, srb)), -2,
              "hrn_shift_add: views and view_masks must not alias out (only base may be out itself)");
    HRN_CHECK(!base || base == out || !overlaps(base, srb, out, srb), -2, "hrn_shift_add: base must be out itself or apart from it");
    HRN_CHECK(!weight || (!overlaps(weight, srb, out, srb) && !(base && overlaps(weight, srb, base, srb)) && !overlaps(views, lrb, weight, srb) &&
                          !(view_masks && overlaps(view_masks, lrb, weight, srb))),
              -2, "hrn_shift_add: weight must not alias another argument");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B;
    HrnProfScope prof("shift_add", 0.0, 4.0 * ((double)lr * (view_masks ? 2 : 1) + (double)sr * (1 + (base ? 1 : 0) + (weight ? 1 : 0))), stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL(shift_add_kernel<decltype(s)::value>, grid, block, 0, stream, views, view_masks, alphas, shifts, base, out, weight,
                           tiles, V, H, W, tx, ty, sigma, prior);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_shift_add_backward(const float* d_out, const float* weight, const float* view_masks, const float* alphas,
                                      const float* shifts, float* d_views, float* d_base, int B, int V, int H, int W, int scale, float sigma,
                                      float prior, void* stream_) {
    HRN_CHECK(d_out && weight && shifts, -2, "hrn_shift_add_backward: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_shift_add_backward", B, V, H, W, scale, sigma, prior, &tx, &ty)) return -2;
    const size_t lr = (size_t)B * V * H * W, sr = (size_t)B * H * W * scale * scale, lrb = lr * sizeof(float), srb = sr * sizeof(float);
    HRN_CHECK(!d_views || (!overlaps(d_views, lrb, d_out, srb) && !overlaps(d_views, lrb, weight, srb) &&
                           !(view_masks && overlaps(d_views, lrb, view_masks, lrb))),
              -2, "hrn_shift_add_backward: d_views must not alias an input");
    HRN_CHECK(!d_base || (!overlaps(d_base, srb, d_out, srb) && !overlaps(d_base, srb, weight, srb) && !(d_views && overlaps(d_base, srb, d_views, lrb))),
              -2, "hrn_shift_add_backward: d_base must not alias d_out, weight or d_views");
    hipStream_t stream = (hipStream_t)stream_;
    HrnProfScope prof("shift_add_backward", 0.0, 4.0 * ((d_views ? (double)lr * (view_masks ? 2 : 1) : 0.0) + (double)sr * (2 + (d_base ? 1 : 0))), stream);
    if (d_views) {
        const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
        const dim3 grid(blocks_for(tiles)), block(kThreads);
        hrn_by_scale(scale, [&](auto s) {
            hipLaunchKernelGGL(shift_add_bwd_views_kernel<decltype(s)::value>, grid, block, 0, stream, d_out, weight, view_masks, alphas, shifts,
                               d_views, tiles, V, H, W, tx, ty, sigma, prior);
        });
        HRN_LAUNCH_CHECK();
    }
    if (d_base) {
        const size_t blocks = (sr + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(shift_add_bwd_base_kernel, dim3(blocks_for(blocks)), dim3(kThreads), 0, stream, d_out, weight, d_base, sr, prior);
        HRN_LAUNCH_CHECK();
    }
    return 0;
}
