// Tiled inference (HRNet.forward_tiled): the two steps around the forward of a chunk of windows.
//   hrn_tile_gather   lrs (B,V,H,W) -> out (w1-w0, B, V, t, t), window-major: out[i][n] = lrs[n][y0 .. y0+t)[x0 .. x0+t) of window w0 + i
//   hrn_tile_scatter  srs (w1-w0, B, 1, St, St) -> the CORES of those windows in out (B, 1, SH, SW); nothing else of out is touched
// with the window rule of hrnet_hip/tiling.py.  Along an axis of length L, with k = t - 2R, window i has
//     core_lo = i == 0 ? 0 : (t - R) + (i - 1) k,   start = min(max(core_lo - R, 0), L - t),   core_hi = start + t == L ? L : start + t - R
// and there are 1 (L == t) or ceil((L - 2R) / k) of them; a scene's windows are the row-major product of its two axes.  The cores
// partition the scene, so every output pixel is written by exactly one window: no atomics, deterministic, and pure data movement -
// tiling.gather / tiling.scatter restate both kernels bit for bit.  The geometry is computed ON THE DEVICE from (H, W, t, R, window
// index) with the arithmetic above: no plan table, no upload, so a call only enqueues one launch and stays graph-capturable.
//
// Both kernels are one row copy.  A row is t floats of a window (gather) or S (cx1 - cx0) floats of a core row (scatter); a group of
// LPR lanes (8, 16, 32 or 64, the power of two that covers a typical row in one step where one exists) owns a row, a block of 256
// threads 256 / LPR rows, rows are grid-strided.  Window origins and core offsets are arbitrary, S = 3 makes most rows start off a 16-byte
// boundary, and W % 4 != 0 shifts every row against the one before, so the path is chosen PER ROW, from the two row addresses:
//   vector   source and destination are equally misaligned (address / 4 mod 4 agrees): h = (4 - that) % 4 head elements one by one
//            (by the group's last lane), then 16-byte loads and stores, slot j = elements h + 4 j .. + 3, then the tail one by one.
//   element  otherwise: the same slots with h = 0, every element by a 4-byte load and store.
// A lane handles slots lane, lane + LPR, ..; the branch on the path is uniform over the LPR lanes of a row.
// Scatter rows run over all St rows of a window; the rows above and below the core return at once (at most 2 S R of S t).
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage):
//   gather_kernel   34 VGPRs, no LDS    scatter_kernel  34 VGPRs, no LDS
// Neither uses scratch (0 bytes / lane, no spills).
#include "../../../include/hrnet_hip.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 1u << 20;                // rows are grid-strided beyond this
constexpr size_t kMaxRows = (size_t)1 << 31;             // per launch, exclusive: row + gridDim.x * rows-per-block stays inside 32 bits

struct Axis { int start, lo, hi; };

// window i of an axis of length L (header comment; tiling.axis_plan)
__host__ __device__ __forceinline__ Axis axis_window(int L, int t, int R, int i) {
    Axis a;
    a.lo = i == 0 ? 0 : (t - R) + (i - 1) * (t - 2 * R);
    const int s = a.lo - R > 0 ? a.lo - R : 0;
    a.start = s < L - t ? s : L - t;
    a.hi = a.start + t == L ? L : a.start + t - R;
    return a;
}

int axis_count(int L, int t, int R) { return L == t ? 1 : (L - 2 * R + (t - 2 * R) - 1) / (t - 2 * R); }

// n floats src -> dst by the `lpr` lanes of a row group, this lane being number `lane` of them
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int n, int lane, int lpr) {
    const unsigned as = (unsigned)((uintptr_t)src >> 2) & 3u, ad = (unsigned)((uintptr_t)dst >> 2) & 3u;
    const bool vec = as == ad;
    const int h = vec ? (int)((4u - as) & 3u) : 0;           // elements in front of the first 16-byte boundary
    if (lane == lpr - 1)
        for (int e = 0; e < min(h, n); ++e) dst[e] = src[e];
    for (int e0 = h + 4 * lane; e0 < n; e0 += 4 * lpr) {
        if (vec && e0 + 4 <= n) {
            *(f32x4*)(dst + e0) = *(const f32x4*)(src + e0);
        } else {
            for (int e = e0; e < min(e0 + 4, n); ++e) dst[e] = src[e];
        }
    }
}

__global__ __launch_bounds__(kThreads) void gather_kernel(const float* __restrict__ lrs, int N, int H, int W, int t, int R, int nx, int w0,
                                                          unsigned rows, int lpr, float* __restrict__ out) {
    const int lane = threadIdx.x & (lpr - 1);
    const unsigned rpb = kThreads / lpr;                     // a power of two
    for (unsigned row = blockIdx.x * rpb + (threadIdx.x >> __builtin_ctz((unsigned)lpr)); row < rows; row += gridDim.x * rpb) {
        const unsigned wn = row / (unsigned)t;               // (window - w0) * N + plane
        const int r = (int)(row - wn * t), i = (int)(wn / (unsigned)N), n = (int)(wn - (unsigned)i * N), w = w0 + i;
        const Axis ay = axis_window(H, t, R, w / nx), ax = axis_window(W, t, R, w % nx);
        copy_row(lrs + (size_t)n * H * W + (size_t)(ay.start + r) * W + ax.start, out + (size_t)row * t, t, lane, lpr);
    }
}

// SH = S H, SW = S W, St = S t
__global__ __launch_bounds__(kThreads) void scatter_kernel(const float* __restrict__ srs, int B, int H, int W, int t, int R, int S, int nx,
                                                           int w0, unsigned rows, int lpr, float* __restrict__ out) {
    const int lane = threadIdx.x & (lpr - 1);
    const unsigned rpb = kThreads / lpr;                     // a power of two
    const int St = S * t, SW = S * W;
    for (unsigned row = blockIdx.x * rpb + (threadIdx.x >> __builtin_ctz((unsigned)lpr)); row < rows; row += gridDim.x * rpb) {
        const unsigned wb = row / (unsigned)St;              // (window - w0) * B + sample
        const int r = (int)(row - wb * St), i = (int)(wb / (unsigned)B), b = (int)(wb - (unsigned)i * B), w = w0 + i;
        const Axis ay = axis_window(H, t, R, w / nx);
        if (r < S * (ay.lo - ay.start) || r >= S * (ay.hi - ay.start)) continue;       // above or below the core
        const Axis ax = axis_window(W, t, R, w % nx);
        copy_row(srs + (size_t)row * St + S * (ax.lo - ax.start), out + (size_t)b * S * H * SW + (size_t)(S * ay.start + r) * SW + S * ax.lo,
                 S * (ax.hi - ax.lo), lane, lpr);
    }
}

// Everything about the plan that can be refused.  -> the number of windows (>= 1) and nx, or a negative code.
int check_plan(const char* fn, int H, int W, int t, int R, int* nx) {
    HRN_CHECK(H > 0 && W > 0 && t > 0 && R >= 0, -2, "%s: bad geometry H=%d W=%d t=%d R=%d", fn, H, W, t, R);
    HRN_CHECK(t <= H && t <= W, -2, "%s: window side t=%d exceeds the scene (H=%d W=%d): a window must lie inside it", fn, t, H, W);
    HRN_CHECK((H == t && W == t) || t >= 2 * R + 1, -2,
              "%s: H=%d W=%d needs more than one window of side t=%d, which must be at least 2R+1 = %d (R=%d)", fn, H, W, t, 2 * R + 1, R);
    HRN_CHECK((size_t)H * W <= (size_t)INT32_MAX, -2, "%s: H=%d x W=%d is beyond 32-bit in-plane offsets", fn, H, W);
    const size_t ny = (size_t)axis_count(H, t, R), nxx = (size_t)axis_count(W, t, R);
    HRN_CHECK(ny * nxx <= (size_t)INT32_MAX, -2, "%s: H=%d W=%d t=%d R=%d gives more than 2^31 - 1 windows", fn, H, W, t, R);
    *nx = (int)nxx;
    return (int)(ny * nxx);
}

int check_range(const char* fn, int w0, int w1, int count) {
    HRN_CHECK(0 <= w0 && w0 < w1 && w1 <= count, -2, "%s: window range [%d, %d) is outside the plan's [0, %d)", fn, w0, w1, count);
    return 0;
}

// lanes per row: the power of two in 8..64 that covers a row of `row_elems` in one step, where one exists
int lanes_per_row(int row_elems) {
    const int slots = (row_elems + 3) / 4;
    int lpr = 8;
    while (lpr < 64 && lpr < slots) lpr *= 2;
    return lpr;
}

unsigned blocks_for(size_t rows, int lpr) {
    const size_t want = (rows + kThreads / lpr - 1) / (kThreads / lpr);
    return (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
}

}  // namespace

extern "C" int hrn_hrnet_halo(int num_layers, int V) {
    HRN_CHECK(num_layers >= 0 && num_layers <= HRN_MAX_RES_LAYERS && V >= 1, -2, "hrn_hrnet_halo: num_layers %d must be in 0..%d and V=%d positive",
              num_layers, HRN_MAX_RES_LAYERS, V);
    int levels = 0;
    for (int n = V; n / 2 > 0; n /= 2) ++levels;
    return 2 + 2 * num_layers + 3 * levels;
}

extern "C" int hrn_tile_count(int H, int W, int t, int R) {
    int nx;
    return check_plan("hrn_tile_count", H, W, t, R, &nx);
}

extern "C" int hrn_tile_gather(const float* lrs, int B, int V, int H, int W, int t, int R, int w0, int w1, float* out, void* stream) {
    const char* fn = "hrn_tile_gather";
    HRN_CHECK(lrs && out, -2, "%s: null argument", fn);
    HRN_CHECK(B > 0 && V > 0 && (size_t)B * V <= (size_t)INT32_MAX, -2, "%s: bad shape B=%d V=%d", fn, B, V);
    int nx;
    const int count = check_plan(fn, H, W, t, R, &nx);
    if (count < 0) return count;
    if (int rc = check_range(fn, w0, w1, count)) return rc;
    const size_t rows = (size_t)(w1 - w0) * B * V * t;
    HRN_CHECK(rows < kMaxRows, -2, "%s: %zu rows of windows in one launch (limit 2^31 - 1): split the window range", fn, rows);
    const int lpr = lanes_per_row(t);
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(rows, lpr)), dim3(kThreads), 0, (hipStream_t)stream, lrs, B * V, H, W, t, R, nx, w0,
                       (unsigned)rows, lpr, out);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_tile_scatter(const float* srs, int B, int H, int W, int t, int R, int scale, int w0, int w1, float* out, void* stream) {
    const char* fn = "hrn_tile_scatter";
    HRN_CHECK(srs && out, -2, "%s: null argument", fn);
    HRN_CHECK(B > 0, -2, "%s: bad shape B=%d", fn, B);
    HRN_CHECK(hrn_scale_ok(scale), -2, "%s: scale must be 2, 3 or 4 (got %d)", fn, scale);
    int nx;
    const int count = check_plan(fn, H, W, t, R, &nx);
    if (count < 0) return count;
    if (int rc = check_range(fn, w0, w1, count)) return rc;
    HRN_CHECK((size_t)scale * H * scale * W <= (size_t)INT32_MAX, -2, "%s: the x%d plane of H=%d x W=%d is beyond 32-bit in-plane offsets", fn,
              scale, H, W);
    const size_t rows = (size_t)(w1 - w0) * B * scale * t;
    HRN_CHECK(rows < kMaxRows, -2, "%s: %zu rows of windows in one launch (limit 2^31 - 1): split the window range", fn, rows);
    const int lpr = lanes_per_row(scale * (W == t ? t : t - 2 * R));        // an inner window's core row; rows at the borders take a second step
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(rows, lpr)), dim3(kThreads), 0, (hipStream_t)stream, srs, B, H, W, t, R, scale, nx, w0,
                       (unsigned)rows, lpr, out);
    HRN_LAUNCH_CHECK();
    return 0;
}
