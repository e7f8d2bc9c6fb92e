// Bicubic x2 / x3 / x4 interpolation of f32 planes with an optional add, and its adjoint (hrn_upsample / hrn_upsample_backward; the
// definition is in include/hrnet_hip.h).  (No counterpart in the reference, whose network synthesises the whole
// image.)  Both kernels are separable passes through LDS over a tile of TH x TW = 8 x 32 LR pixels per workgroup of 256 threads; a
// workgroup walks tiles (plane-major) with a grid stride, so any number of planes goes through one launch (the tile, its walk and the
// limits of a side: lr_tile.h, which shift_add.hip and observe.hip share).  The S x 4 tap weights come by
// value (computed on the host in fp64, rounded to fp32): a phase's weights are scalars, and every tap index below is a compile-time
// constant after unrolling - no array is indexed by a run-time value, no scratch.
//
// With S the scale, output index j = S m + p (cell m, phase p) reads the taps i - 1 .. i + 2, i = m + d_p, d_p = -1 for 2 p + 1 < S and 0
// otherwise: an output row or column of cell m touches the five source cells m - 2 .. m + 2.
//
// Forward, per tile:
//   1. raw[TH + 4][TW + 4]  <- the tile plus a halo of two, row and column indices clamped to the plane AT THE LOAD: no border branch later
//   2. hbuf[TH + 4][S TW]   <- the column taps: h = w0 f0, then fma(w1 f1), fma(w2 f2), fma(w3 f3) - taps ascending
//   3. a thread takes an LR row y and four output columns: five 16-byte LDS reads (rows y - 2 .. y + 2 of hbuf), then per phase the row
//      taps in the same ascending fma chain, the add of `base`, and one 16-byte store where the output row starts on a 16-byte boundary
//      (out and base alike; the choice is per row, as in tile.hip) and the four columns are inside the plane; single stores elsewhere.
//      `base` is read by the thread that writes the same elements, so base == out is an in-place add.
// Backward, per tile: the adjoint as a gather.  An LR pixel sums, over the virtual indices u that the clamp folds onto it (u = its own
// index; at a border also the two beyond the edge; with a side below 3 several of them), the output gradients of cells u - 2 .. u + 2
// with the weight of tap c = u + 1 - m - d_p - the terms j ascending, u ascending, one fma each.
//   1. gs[(TH + 4) S][(TW + 4) S]  <- the output gradients of cells y0 - 2 .. y0 + TH + 1 (likewise columns), zero outside the plane;
//                                     a wave loads whole rows with 16-byte loads (the bytes are 1.7 x d_out's: the halo)
//   2. tv[TH][(TW + 4) S]          <- the row gather of every staged column
//   3. d_frames                    <- the column gather of tv
// A cell outside the staged range is always outside the plane (the folds reach at most two cells past a border pixel), so it is skipped.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are stated in DESIGN.md section 7r.
#include "lr_tile.h"

#include <cmath>

namespace {

struct UpWeights { float w[4][4]; };                     // [phase][tap], phases 0 .. S - 1

template <int S> __host__ __device__ constexpr int phase_shift(int p) { return 2 * p + 1 < S ? -1 : 0; }

// taps ascending: w0 f0, then one fma per further tap
__device__ __forceinline__ float taps4(const float (&w)[4], float f0, float f1, float f2, float f3) {
    return fmaf(w[3], f3, fmaf(w[2], f2, fmaf(w[1], f1, w[0] * f0)));
}

// base and out may be the same pointer (no __restrict__ on either)
template <int S>
__global__ __launch_bounds__(kThreads) void upsample_kernel(const float* __restrict__ frames, const float* base, float* out, size_t tiles,
                                                            int H, int W, unsigned tiles_x, unsigned tiles_y, UpWeights wt) {
    constexpr int RH = kTH + 4, RW = kTW + 4, HW_ = S * kTW, VPR = HW_ / 4;
    __shared__ float raw[RH][RW];
    __shared__ __attribute__((aligned(16))) float hbuf[RH][HW_];
    const int SH = S * H, SW = S * W, tid = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);
        const float* src = frames + tp.n * (size_t)H * W;
        for (int e = tid; e < RH * RW; e += kThreads) {
            const int r = e / RW, c = e - r * RW;
            const int gy = min(max(tp.y0 + r - 2, 0), H - 1), gx = min(max(tp.x0 + c - 2, 0), W - 1);
            raw[r][c] = src[(size_t)gy * W + gx];
        }
        __syncthreads();
        for (int e = tid; e < RH * kTW; e += kThreads) {
            const int r = e / kTW, x = e - r * kTW;
            float f[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = raw[r][x + k];           // source columns x - 2 .. x + 2 of the tile
#pragma unroll
            for (int p = 0; p < S; ++p) {
                const int d = phase_shift<S>(p);
                hbuf[r][S * x + p] = taps4(wt.w[p], f[d + 1], f[d + 2], f[d + 3], f[d + 4]);
            }
        }
        __syncthreads();
        for (int e = tid; e < kTH * VPR; e += kThreads) {
            const int y = e / VPR, c4 = e - y * VPR;
            const int ox = S * tp.x0 + 4 * c4;
            if (tp.y0 + y >= H || ox >= SW) continue;
            f32x4 h[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) h[k] = *(const f32x4*)&hbuf[y + k][4 * c4];     // source rows y - 2 .. y + 2 of the tile
#pragma unroll
            for (int p = 0; p < S; ++p) {
                const int d = phase_shift<S>(p);
                f32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = taps4(wt.w[p], h[d + 1][k], h[d + 2][k], h[d + 3][k], h[d + 4][k]);
                const size_t row = (tp.n * (size_t)SH + (size_t)(S * (tp.y0 + y) + p)) * (size_t)SW;
                float* orow = out + row;
                const float* brow = base ? base + row : nullptr;
                const bool vec = ox + 4 <= SW && ((uintptr_t)orow & 15u) == 0 && ((uintptr_t)brow & 15u) == 0;
                if (vec) {
                    if (brow) v += *(const f32x4*)(brow + ox);
                    *(f32x4*)(orow + ox) = v;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ox + k < SW) orow[ox + k] = brow ? brow[ox + k] + v[k] : v[k];
                }
            }
        }
        // (the next tile's raw is not read before its first barrier, its hbuf not written before that barrier either)
    }
}

// One virtual index u of the gather along an axis: the cells u - 2 .. u + 2, k0 = u - 2 - (the first staged cell).  CHECK: skip the
// cells outside the `cells` staged ones (they are outside the plane).
template <int S, bool CHECK, class At>
__device__ __forceinline__ float gather_cells(const UpWeights& wt, float acc, int k0, int cells, At at) {
#pragma unroll
    for (int dm = -2; dm <= 2; ++dm) {
        const int k = k0 + 2 + dm;
        if (CHECK && (k < 0 || k >= cells)) continue;
#pragma unroll
        for (int p = 0; p < S; ++p) {
            const int c = 1 - dm - phase_shift<S>(p);
            if (c >= 0 && c <= 3) acc = fmaf(wt.w[p][c], at(k, p), acc);
        }
    }
    return acc;
}

// The gather along one axis: the sum over the virtual indices u folding onto index X of an axis of length L, of cells u - 2 .. u + 2.
// cell0: the first staged cell; cells: how many are staged; at(cell - cell0, p): the staged value of that cell's phase p.  An inner
// index is its own u alone and all its five cells are staged: the same terms in the same order, without the checks.
template <int S, class At>
__device__ __forceinline__ float fold_gather(const UpWeights& wt, int X, int L, int cell0, int cells, At at) {
    if (X > 0 && X < L - 1) return gather_cells<S, false>(wt, 0.f, X - 2 - cell0, cells, at);
    const int lo = X == 0 ? -2 : X, hi = X == L - 1 ? L + 1 : X;
    float acc = 0.f;
    for (int u = lo; u <= hi; ++u) acc = gather_cells<S, true>(wt, acc, u - 2 - cell0, cells, at);
    return acc;
}

template <int S>
__global__ __launch_bounds__(kThreads) void upsample_bwd_kernel(const float* __restrict__ d_out, float* __restrict__ d_frames, size_t tiles,
                                                                int H, int W, unsigned tiles_x, unsigned tiles_y, UpWeights wt) {
    constexpr int CY = kTH + 4, CX = kTW + 4, GR = CY * S, GC = CX * S;
    constexpr int RPW = GR / (kThreads / 64);                               // rows of gs a wave stages
    static_assert((GC + 6) / 4 <= 64 && GR % (kThreads / 64) == 0, "a wave stages a row of gs in one step, and whole rows");
    __shared__ float gs[GR][GC];
    __shared__ float tv[kTH][GC];
    const int SH = S * H, SW = S * W, tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);
        const float* g = d_out + tp.n * (size_t)SH * SW;
        const int oy0 = S * (tp.y0 - 2), ox0 = S * (tp.x0 - 2);
        // A wave takes whole rows (the row's validity, address and alignment are scalars); a lane takes the four elements that start
        // on a 16-byte boundary of the row's memory: one 16-byte load where they all lie inside the row, single loads at its ends.
        // All of a wave's RPW rows are loaded before the first is written to LDS: RPW loads in flight per lane, not one.
        f32x4 v[RPW];
        int ox[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int oy = oy0 + wave + i * (kThreads / 64);
            const bool row_ok = oy >= 0 && oy < SH;
            const float* grow = g + (size_t)(row_ok ? oy : 0) * SW;
            const int mis = (int)(((uintptr_t)grow >> 2) & 3u);         // the row's element 0 lies `mis` elements past a 16-byte boundary
            ox[i] = ox0 - ((ox0 + mis) & 3) + 4 * lane;                 // (ox + mis) % 4 == 0, and the first lane reaches ox0
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row_ok && ox[i] < ox0 + GC) {
                if (ox[i] >= 0 && ox[i] + 4 <= SW) {
                    v[i] = *(const f32x4*)(grow + ox[i]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ox[i] + k >= 0 && ox[i] + k < SW) v[i][k] = grow[ox[i] + k];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = ox[i] + k - ox0;
                if (c >= 0 && c < GC) gs[wave + i * (kThreads / 64)][c] = v[i][k];
            }
        }
        __syncthreads();
        for (int e = tid; e < kTH * GC; e += kThreads) {
            const int y = e / GC, q = e - y * GC;
            if (tp.y0 + y >= H) continue;
            tv[y][q] = fold_gather<S>(wt, tp.y0 + y, H, tp.y0 - 2, CY, [&](int k, int p) { return gs[k * S + p][q]; });
        }
        __syncthreads();
        {
            const int y = tid / kTW, x = tid - y * kTW;                  // kThreads == kTH * kTW
            if (tp.y0 + y < H && tp.x0 + x < W)
                d_frames[tp.n * (size_t)H * W + (size_t)(tp.y0 + y) * W + (tp.x0 + x)] =
                    fold_gather<S>(wt, tp.x0 + x, W, tp.x0 - 2, CX, [&](int k, int p) { return tv[y][k * S + p]; });
        }
        __syncthreads();                                                // tv and gs are free for the next tile
    }
}

// Keys' cubic with parameter a: the weights of the taps i - 1 .. i + 2 at every phase, fp64 rounded to fp32 (hrnet_hip/upsample.py
// restates this table)
UpWeights phase_weights(int S, float a_) {
    const double a = (double)a_;
    auto w1 = [a](double x) { return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0; };
    auto w2 = [a](double x) { return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a; };
    UpWeights w = {};
    for (int p = 0; p < S; ++p) {
        const double x = (p + 0.5) / S - 0.5, t = x - std::floor(x);
        w.w[p][0] = (float)w2(t + 1.0);
        w.w[p][1] = (float)w1(t);
        w.w[p][2] = (float)w1(1.0 - t);
        w.w[p][3] = (float)w2(2.0 - t);
    }
    return w;
}

// what both entry points refuse; -> the number of tiles, or 0 with the error set
size_t check_shape(const char* fn, int64_t n_planes, int H, int W, int scale, float a, unsigned* tiles_x, unsigned* tiles_y) {
    *tiles_x = *tiles_y = 0;
    if (!(n_planes > 0 && H > 0 && W > 0)) { hrn_set_error("%s: empty input n_planes=%lld H=%d W=%d", fn, (long long)n_planes, H, W); return 0; }
    if (!check_side_scale(fn, "planes", H, W, scale)) return 0;
    if (!std::isfinite(a)) { hrn_set_error("%s: the kernel parameter a must be finite", fn); return 0; }
    // 2^62 elements (shift_add.hip's limit too; observe.hip stops at 2^60; no reason for the difference is recorded)
    if ((size_t)n_planes > ((size_t)1 << 62) / ((size_t)scale * scale * H * W)) {
        hrn_set_error("%s: %lld planes of %d x %d exceed the address space", fn, (long long)n_planes, H, W);
        return 0;
    }
    return plane_tiles(H, W, tiles_x, tiles_y) * (size_t)n_planes;
}

}  // namespace

extern "C" int hrn_upsample(const float* frames, const float* base, float* out, int64_t n_planes, int H, int W, int scale, float a,
                            void* stream_) {
    HRN_CHECK(frames && out, -2, "hrn_upsample: null argument");
    unsigned tx, ty;
    const size_t tiles = check_shape("hrn_upsample", n_planes, H, W, scale, a, &tx, &ty);
    if (!tiles) return -2;
    const size_t lr = (size_t)n_planes * H * W, lrb = lr * sizeof(float), srb = lrb * scale * scale;
    HRN_CHECK(!overlaps(frames, lrb, out, srb), -2, "hrn_upsample: frames must not alias out (only base may be out itself)");
    HRN_CHECK(!base || base == out || !overlaps(base, srb, out, srb), -2, "hrn_upsample: base must be out itself or apart from it");
    hipStream_t stream = (hipStream_t)stream_;
    const UpWeights wt = phase_weights(scale, a);
    HrnProfScope prof("upsample", 0.0, (double)lr * 4 * (1 + (base ? 2 : 1) * scale * scale), stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL(upsample_kernel<decltype(s)::value>, grid, block, 0, stream, frames, base, out, tiles, H, W, tx, ty, wt);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_upsample_backward(const float* d_out, float* d_frames, int64_t n_planes, int H, int W, int scale, float a, void* stream_) {
    HRN_CHECK(d_out && d_frames, -2, "hrn_upsample_backward: null argument");
    unsigned tx, ty;
    const size_t tiles = check_shape("hrn_upsample_backward", n_planes, H, W, scale, a, &tx, &ty);
    if (!tiles) return -2;
    const size_t lr = (size_t)n_planes * H * W, lrb = lr * sizeof(float), srb = lrb * scale * scale;
    HRN_CHECK(!overlaps(d_frames, lrb, d_out, srb), -2, "hrn_upsample_backward: d_frames must not alias d_out");
    hipStream_t stream = (hipStream_t)stream_;
    const UpWeights wt = phase_weights(scale, a);
    HrnProfScope prof("upsample_backward", 0.0, (double)lr * 4 * (1 + scale * scale), stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL(upsample_bwd_kernel<decltype(s)::value>, grid, block, 0, stream, d_out, d_frames, tiles, H, W, tx, ty, wt);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}
