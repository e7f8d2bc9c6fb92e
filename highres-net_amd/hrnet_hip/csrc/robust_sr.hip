// A robust data term and a bilateral-TV prior for the reconstruction on the HR grid (hrn_robust_sums, hrn_robust_finish,
// hrn_robust_apply, hrn_btv_step, hrn_btv_backward, hrn_btv_value; the definition is in include/hrnet_hip.h).
// (No counterpart in the reference.)
//
// Robust data term: the residual e of hrn_consistency_residual is re-weighted with the Welsch weight w = exp(-((e + beta_prev) / delta)^2)
// where counted - counted is sample_counted of observe_geom.h, the decision the residual kernel and the adjoint take.
//   sums:   a workgroup of 256 threads owns the 8 x 32 samples of one view's tile (lr_tile.h), a thread per sample; the tile's fp64
//           partials of sum w, sum w e, sum w (e + beta_prev)^2: lanes by xor exchanges, the four waves in order.
//   finish: one workgroup per sample, a wave per view adds that view's tiles (a lane every 64th tile in index order, the lanes by xor
//           exchanges), thread 0 adds the views in index order: beta, the inlier fraction, the weighted loss.
//   apply:  r' = w (e + beta) elementwise, w recomputed, into a second plane that hrn_observe_adjoint takes with beta = NULL.
//
// Bilateral TV: g_p = 2 sum_q w_{|l| + |m|} phi'(x_p - x_q) over the (2 P + 1)^2 - 1 neighbours q = p + (l, m) inside the frame, which is
// the definition's sum_d w_d [phi'(x_p - x_{p-d}) - phi'(x_{p+d} - x_p)] (phi' is odd and fp32 negation exact; d and -d are both in the
// sum), the terms in raster order of (l, m), one fma each.
//   A workgroup of 256 threads owns a 16 x 64 HR tile (2 x 2 HR pixels per cell of lr_tile.h's 8 x 32 walk).
//   1. win[16 + 2 P][72]  <- rows y0 - P .. y0 + 15 + P, columns x0 - 4 .. x0 + 67, zero outside the frame: a thread loads 16 bytes that
//      start on a 16-byte boundary of the row's memory (the row's misalignment is taken per row, so odd widths keep vector loads), single
//      loads where the four cross the frame's edge; all of a thread's loads are issued before its first LDS write.
//   2. a thread owns one column and 4 consecutive rows: its (4 + 2 P) x (2 P + 1) window goes to registers with ds_read_b32.  A half-wave
//      reads 32 consecutive words of one LDS row for every tap: 32 distinct banks, NO conflict, whatever the row stride.
//      The staging writes are ds_write_b32 at a stride of 4 words within a row of 19 chunks, so a half-wave meets 8 of the 32 banks:
//      4-way (3.8 .. 4.0 on average over the half-waves, counted from the addresses).  They are 8 of a
//      thread's LDS instructions against the 40 tap reads at P = 2.
//   3. step: out = x - c_b g; backward: out = gain_b g; value: the tile's fp64 partial of sum_p sum_q w phi(x_p - x_q) (every unordered
//      pair twice, as the definition has it), then a finish launch that adds a plane's tiles in a fixed order.
//   P is a template parameter, the taps fully unrolled; out must not be x (a stencil).
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are stated in DESIGN.md section 7u.
#include "observe_geom.h"

#include <cmath>

namespace {

constexpr int kRobustFinishThreads = 1024;
constexpr double kMinWeight = 0x1p-60;                   // a weight sum below this is "nothing counts"

// w of one sample: counted exp(-((e + beta_prev) / delta)^2), fp32
__device__ __forceinline__ float welsch(bool counted, float e, float bp, float delta) {
    const float u = (e + bp) / delta;
    return counted ? expf(-(u * u)) : 0.f;
}

// ----------------------------------------------------------------------------- robust sums / apply
// APPLY false: the tile's partials.  true: out = w (e + beta).
template <int S, bool APPLY>
__global__ __launch_bounds__(kThreads) void robust_kernel(const float* __restrict__ res, const float* __restrict__ masks,
                                                          const float* __restrict__ alphas, const float* __restrict__ shifts,
                                                          const float* __restrict__ beta_prev, const float* __restrict__ beta,
                                                          float* __restrict__ out, double* __restrict__ partials, float delta, size_t tiles,
                                                          int H, int W, unsigned tiles_x, unsigned tiles_y) {
    __shared__ double red[kThreads / 64][3];
    const int tid = threadIdx.x, ty = tid / kTW, tx = tid - ty * kTW;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);         // tp.n: the view's plane, b V + v
        const int iy = tp.y0 + ty, ix = tp.x0 + tx;
        const bool inside = iy < H && ix < W;
        const size_t at = tp.n * (size_t)H * W + (size_t)(inside ? iy : 0) * W + (inside ? ix : 0);
        const ViewGeom g = view_geom<S>(alphas, shifts, tp.n);       // uniform
        const bool counted = inside && sample_counted<S>(g, masks, at, iy, ix, H, W);
        const float e = counted ? res[at] : 0.f, bp = beta_prev[tp.n];
        const float w = welsch(counted, e, bp, delta);
        if (APPLY) {
            if (inside) out[at] = counted ? w * (e + beta[tp.n]) : 0.f;
        } else {
            const double wd = (double)w, ed = (double)e, rd = (double)e + (double)bp;
            double v0 = wd, v1 = wd * ed, v2 = wd * rd * rd;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                v0 += __shfl_xor(v0, m);
                v1 += __shfl_xor(v1, m);
                v2 += __shfl_xor(v2, m);
            }
            __syncthreads();                                         // the previous tile's reads of red are done
            if ((tid & 63) == 0) { red[tid / 64][0] = v0; red[tid / 64][1] = v1; red[tid / 64][2] = v2; }
            __syncthreads();
            if (tid < 3) {
                double t = red[0][tid];
#pragma unroll
                for (int wv = 1; wv < kThreads / 64; ++wv) t += red[wv][tid];
                partials[3 * tile + tid] = t;
            }
        }
    }
}

// block b = sample b, a wave per view, kRobustFinishThreads / 64 views a round
__global__ __launch_bounds__(kRobustFinishThreads) void robust_finish_kernel(const double* __restrict__ partials, const int* __restrict__ count,
                                                                             float* __restrict__ beta, float* __restrict__ inlier,
                                                                             float* __restrict__ loss, int V, size_t per_view, int brightness) {
    constexpr int WAVES = kRobustFinishThreads / 64;
    __shared__ double round_w[WAVES], round_q[WAVES];
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double w_all = 0.0, q_all = 0.0;                     // thread 0's: the views in index order
    for (int v0 = 0; v0 < V; v0 += WAVES) {
        const int v = v0 + wave;
        if (v < V) {
            const size_t bv = b * (size_t)V + (size_t)v;
            const double* p = partials + 3 * bv * per_view;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4
            for (size_t t = lane; t < per_view; t += 64) { s0 += p[3 * t]; s1 += p[3 * t + 1]; s2 += p[3 * t + 2]; }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                s0 += __shfl_xor(s0, m);
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (lane == 0) {
                const int n = count[bv];
                beta[bv] = brightness && s0 >= kMinWeight ? (float)(-s1 / s0) : 0.f;
                inlier[bv] = n > 0 ? (float)(s0 / (double)n) : 0.f;
                round_w[wave] = s0;
                round_q[wave] = s2;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < WAVES && v0 + w < V; ++w) { w_all += round_w[w]; q_all += round_q[w]; }
        __syncthreads();                                 // the round's sums are taken before the next round writes them
    }
    if (threadIdx.x == 0) loss[b] = w_all >= kMinWeight ? (float)(q_all / w_all) : 0.f;
}

// ----------------------------------------------------------------------------- bilateral TV
constexpr int kBH = 2 * kTH, kBW = 2 * kTW;              // the HR tile: 2 x 2 pixels per cell of the 8 x 32 walk
constexpr int kBRows = kBH * kBW / kThreads;             // rows of a thread's column strip
constexpr int kBLW = kBW + 8;                            // an LDS row: columns x0 - 4 .. x0 + kBW + 3
constexpr int kBNC = kBLW / 4 + 1;                       // 16-byte chunks that cover it from any alignment
constexpr int kBtvMaxSide = HRN_BTV_MAX_SIDE;
static_assert(HRN_BTV_TILE_H == kBH && HRN_BTV_TILE_W == kBW && kBRows == 4 && kBW == 64, "a wave is one row of the tile's columns");
static_assert(HRN_BTV_MAX_P <= 4, "the halo fits the four columns left of x0");

struct BtvWeights { float w[2 * HRN_BTV_MAX_P + 1]; };   // alpha^k, k = |l| + |m|: fp64 powers rounded to fp32 once (on the host)

enum { BTV_STEP = 0, BTV_BACKWARD = 1, BTV_VALUE = 2 };

template <int P, int MODE>
__global__ __launch_bounds__(kThreads) void btv_kernel(const float* __restrict__ x, const float* __restrict__ cf, float* __restrict__ out,
                                                       double* __restrict__ partials, BtvWeights wt, float eps, float eps2, size_t tiles,
                                                       int SH, int SW, unsigned tiles_x, unsigned tiles_y) {
    constexpr int WH = kBH + 2 * P, NR = kBRows + 2 * P, NCOL = 2 * P + 1;
    constexpr int LPT = (WH * kBNC + kThreads - 1) / kThreads;
    __shared__ float win[WH][kBLW];
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x, tx = tid & 63, tq = tid >> 6;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);         // tp.n: the plane; cells of 2 x 2 HR pixels
        const int y0 = 2 * tp.y0, x0 = 2 * tp.x0;
        const float* plane = x + tp.n * (size_t)SH * SW;
        f32x4 ld[LPT];
        int u0[LPT];
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int e = tid + i * kThreads, r = e / kBNC, c = e - r * kBNC;
            const int gy = y0 - P + r;
            const bool row_ok = e < WH * kBNC && gy >= 0 && gy < SH;
            const float* row = plane + (size_t)(row_ok ? gy : 0) * SW;
            const int mis = (int)(((uintptr_t)row >> 2) & 3u);       // the row's element 0 lies `mis` elements past a 16-byte boundary
            u0[i] = 4 * c - mis;                                     // the chunk's first column, relative to x0 - 4
            const int gx = x0 - 4 + u0[i];
            ld[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row_ok && gx + 3 >= 0 && gx < SW) {
                if (gx >= 0 && gx + 4 <= SW) ld[i] = *(const f32x4*)(row + gx);
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (gx + k >= 0 && gx + k < SW) ld[i][k] = row[gx + k];
                }
            }
        }
        __syncthreads();                                             // the previous tile's reads of win / red are done
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int e = tid + i * kThreads, r = e / kBNC;
            if (e < WH * kBNC) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (u0[i] + k >= 0 && u0[i] + k < kBLW) win[r][u0[i] + k] = ld[i][k];
            }
        }
        __syncthreads();
        float v[NR][NCOL];
#pragma unroll
        for (int a = 0; a < NR; ++a)
#pragma unroll
            for (int b = 0; b < NCOL; ++b) v[a][b] = win[kBRows * tq + a][tx + 4 - P + b];
        const int gx = x0 + tx, gy0 = y0 + kBRows * tq;
        bool rok[NR], cok[NCOL];
#pragma unroll
        for (int a = 0; a < NR; ++a) rok[a] = gy0 + a - P >= 0 && gy0 + a - P < SH;
#pragma unroll
        for (int b = 0; b < NCOL; ++b) cok[b] = gx + b - P >= 0 && gx + b - P < SW;
        const float c = MODE == BTV_VALUE ? 0.f : cf[tp.n];
        double tsum = 0.0;
#pragma unroll
        for (int j = 0; j < kBRows; ++j) {
            const float xp = v[j + P][P];
            float acc = 0.f;
#pragma unroll
            for (int l = -P; l <= P; ++l)
#pragma unroll
                for (int m = -P; m <= P; ++m) {
                    if (l == 0 && m == 0) continue;
                    const float t = xp - v[j + P + l][P + m];
                    const float q = fmaf(t, t, eps2);
                    const float ph = MODE == BTV_VALUE ? t * t * __builtin_amdgcn_rcpf(sqrtf(q) + eps) : t * rsqrtf(q);
                    const float wk = wt.w[(l < 0 ? -l : l) + (m < 0 ? -m : m)];
                    acc = rok[j + P + l] && cok[P + m] ? fmaf(wk, ph, acc) : acc;
                }
            const bool inside = rok[j + P] && cok[P];
            if (MODE == BTV_VALUE) {
                if (inside) tsum += (double)acc;
            } else if (inside) {
                const size_t at = tp.n * (size_t)SH * SW + (size_t)(gy0 + j) * SW + (size_t)gx;
                const float g = 2.f * acc;
                out[at] = MODE == BTV_STEP ? fmaf(-c, g, xp) : c * g;
            }
        }
        if (MODE == BTV_VALUE) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) tsum += __shfl_xor(tsum, m);
            if (tx == 0) red[tq] = tsum;
            __syncthreads();
            if (tid == 0) {
                double t = red[0];
#pragma unroll
                for (int wv = 1; wv < kThreads / 64; ++wv) t += red[wv];
                partials[tile] = t;
            }
        }
    }
}

// value[p] = gain R_p / (SH SW): block p = plane p; a thread every 256th tile in index order, lanes by xor exchanges, waves in order
__global__ __launch_bounds__(kThreads) void btv_value_finish_kernel(const double* __restrict__ partials, float* __restrict__ value,
                                                                    size_t per_plane, double pixels, float gain) {
    __shared__ double red[kThreads / 64];
    const double* p = partials + (size_t)blockIdx.x * per_plane;
    double s = 0.0;
    for (size_t t = threadIdx.x; t < per_plane; t += kThreads) s += p[t];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int wv = 1; wv < kThreads / 64; ++wv) t += red[wv];
        value[blockIdx.x] = (float)((double)gain * t / pixels);
    }
}

// ----------------------------------------------------------------------------- host checks
bool robust_shape(const char* fn, int B, int V, int H, int W, int scale, unsigned* tiles_x, unsigned* tiles_y) {
    *tiles_x = *tiles_y = 0;
    if (!(B > 0 && V > 0 && H > 0 && W > 0)) { hrn_set_error("%s: empty input B=%d V=%d H=%d W=%d", fn, B, V, H, W); return false; }
    if (!check_side_scale(fn, "frames", H, W, scale)) return false;
    if ((size_t)B > ((size_t)1 << 60) / ((size_t)V * scale * scale * H * W)) {
        hrn_set_error("%s: %d x %d frames of %d x %d exceed the address space", fn, B, V, H, W);
        return false;
    }
    plane_tiles(H, W, tiles_x, tiles_y);
    return true;
}

bool delta_ok(const char* fn, float delta) {
    if (std::isfinite(delta) && delta > 0.f) return true;
    hrn_set_error("%s: delta must be positive and finite (got %g)", fn, (double)delta);
    return false;
}

size_t robust_bytes(int B, int V, int H, int W) { return (size_t)B * V * plane_tiles(H, W) * 3 * sizeof(double); }

// planes of 1..kBtvMaxSide a side, P, alpha, eps -> true with the tiles and the weights, or false with the error set
bool btv_shape(const char* fn, int planes, int SH, int SW, int P, float alpha, float eps, unsigned* tiles_x, unsigned* tiles_y,
               BtvWeights* wt) {
    *tiles_x = *tiles_y = 0;
    if (!(planes > 0 && SH > 0 && SW > 0)) { hrn_set_error("%s: empty input planes=%d SH=%d SW=%d", fn, planes, SH, SW); return false; }
    if (SH > kBtvMaxSide || SW > kBtvMaxSide) { hrn_set_error("%s: planes of 1..%d a side; got SH=%d SW=%d", fn, kBtvMaxSide, SH, SW); return false; }
    if ((size_t)planes > ((size_t)1 << 60) / ((size_t)SH * SW)) { hrn_set_error("%s: %d planes of %d x %d exceed the address space", fn, planes, SH, SW); return false; }
    if (P < 1 || P > HRN_BTV_MAX_P) { hrn_set_error("%s: P must be 1..%d (got %d)", fn, HRN_BTV_MAX_P, P); return false; }
    if (!(std::isfinite(alpha) && alpha > 0.f && alpha <= 1.f)) { hrn_set_error("%s: alpha must lie in (0, 1] (got %g)", fn, (double)alpha); return false; }
    if (!(std::isfinite(eps) && eps > 0.f)) { hrn_set_error("%s: eps must be positive and finite (got %g)", fn, (double)eps); return false; }
    plane_tiles((SH + 1) / 2, (SW + 1) / 2, tiles_x, tiles_y);
    for (int k = 0; k <= 2 * HRN_BTV_MAX_P; ++k) wt->w[k] = (float)std::pow((double)alpha, (double)k);
    return true;
}

size_t btv_bytes(int planes, int SH, int SW) { return (size_t)planes * plane_tiles((SH + 1) / 2, (SW + 1) / 2) * sizeof(double); }

template <int MODE>
void btv_launch(int P, const float* x, const float* cf, float* out, double* partials, const BtvWeights& wt, float eps, size_t tiles, int SH,
                int SW, unsigned tx, unsigned ty, hipStream_t stream) {
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    const float eps2 = (float)((double)eps * (double)eps);
    switch (P) {
        case 1: hipLaunchKernelGGL((btv_kernel<1, MODE>), grid, block, 0, stream, x, cf, out, partials, wt, eps, eps2, tiles, SH, SW, tx, ty); break;
        case 2: hipLaunchKernelGGL((btv_kernel<2, MODE>), grid, block, 0, stream, x, cf, out, partials, wt, eps, eps2, tiles, SH, SW, tx, ty); break;
        default: hipLaunchKernelGGL((btv_kernel<3, MODE>), grid, block, 0, stream, x, cf, out, partials, wt, eps, eps2, tiles, SH, SW, tx, ty); break;
    }
}

// hrn_btv_step (MODE BTV_STEP) and hrn_btv_backward (BTV_BACKWARD): one body
template <int MODE>
int btv_map(const char* fn, const float* x, const float* cf, float* out, int planes, int SH, int SW, int P, float alpha, float eps,
            void* stream_) {
    HRN_CHECK(x && cf && out, -2, "%s: null argument", fn);
    unsigned tx, ty;
    BtvWeights wt;
    if (!btv_shape(fn, planes, SH, SW, P, alpha, eps, &tx, &ty, &wt)) return -2;
    const size_t bytes = (size_t)planes * SH * SW * 4;
    HRN_CHECK(!overlaps(out, bytes, x, bytes) && !overlaps(out, bytes, cf, (size_t)planes * 4), -2,
              "%s: out must not alias x (a stencil: ping-pong two frames) or the coefficients", fn);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)planes;
    HrnProfScope prof(MODE == BTV_STEP ? "btv_step" : "btv_backward", 0.0, 2.0 * (double)bytes, stream);
    btv_launch<MODE>(P, x, cf, out, nullptr, wt, eps, tiles, SH, SW, tx, ty, stream);
    HRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t hrn_robust_workspace_bytes(int B, int V, int H, int W) {
    if (!(B > 0 && V > 0 && H > 0 && W > 0) || H > kMaxSide || W > kMaxSide) return 0;
    return robust_bytes(B, V, H, W);
}

extern "C" int hrn_robust_sums(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta_prev,
                               void* workspace, size_t workspace_bytes, int B, int V, int H, int W, int scale, float delta, void* stream_) {
    HRN_CHECK(residual && shifts && beta_prev && workspace, -2, "hrn_robust_sums: null argument");
    unsigned tx, ty;
    if (!robust_shape("hrn_robust_sums", B, V, H, W, scale, &tx, &ty) || !delta_ok("hrn_robust_sums", delta)) return -2;
    const size_t need = robust_bytes(B, V, H, W);
    HRN_CHECK(workspace_bytes >= need, -2, "hrn_robust_sums: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HRN_CHECK(((uintptr_t)workspace & 7u) == 0, -2, "hrn_robust_sums: workspace must be 8-byte aligned");
    const size_t lr = (size_t)B * V * H * W * 4, sh = (size_t)B * V * 8;
    HRN_CHECK(!overlaps(workspace, need, residual, lr) && !(lr_masks && overlaps(workspace, need, lr_masks, lr)) &&
                  !overlaps(workspace, need, shifts, sh) && !(alphas && overlaps(workspace, need, alphas, sh / 2)) &&
                  !overlaps(workspace, need, beta_prev, sh / 2),
              -2, "hrn_robust_sums: workspace must not alias an input");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("robust_sums", 0.0, (double)lr * (lr_masks ? 2 : 1) + (double)need, stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((robust_kernel<decltype(s)::value, false>), grid, block, 0, stream, residual, lr_masks, alphas, shifts, beta_prev,
                           (const float*)nullptr, (float*)nullptr, (double*)workspace, delta, tiles, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_robust_finish(const void* workspace, size_t workspace_bytes, const int* count, float* beta, float* inlier, float* loss,
                                 int B, int V, int H, int W, int brightness, void* stream_) {
    HRN_CHECK(workspace && count && beta && inlier && loss, -2, "hrn_robust_finish: null argument");
    unsigned tx, ty;
    if (!robust_shape("hrn_robust_finish", B, V, H, W, 2, &tx, &ty)) return -2;
    const size_t need = robust_bytes(B, V, H, W);
    HRN_CHECK(workspace_bytes >= need, -2, "hrn_robust_finish: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HRN_CHECK(((uintptr_t)workspace & 7u) == 0, -2, "hrn_robust_finish: workspace must be 8-byte aligned");
    const size_t bv = (size_t)B * V;
    const void* outs[3] = {beta, inlier, loss};
    const size_t bytes[3] = {bv * 4, bv * 4, (size_t)B * 4};
    for (int i = 0; i < 3; ++i) {
        HRN_CHECK(!overlaps(outs[i], bytes[i], workspace, need) && !overlaps(outs[i], bytes[i], count, bv * 4), -2,
                  "hrn_robust_finish: an output must not alias the workspace or count");
        for (int j = i + 1; j < 3; ++j)
            HRN_CHECK(!overlaps(outs[i], bytes[i], outs[j], bytes[j]), -2, "hrn_robust_finish: the outputs must not alias each other");
    }
    hipStream_t stream = (hipStream_t)stream_;
    HrnProfScope prof("robust_finish", 0.0, (double)need, stream);
    hipLaunchKernelGGL(robust_finish_kernel, dim3((unsigned)B), dim3(kRobustFinishThreads), 0, stream, (const double*)workspace, count, beta,
                       inlier, loss, V, (size_t)tx * ty, brightness ? 1 : 0);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_robust_apply(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta_prev,
                                const float* beta, float* weighted, int B, int V, int H, int W, int scale, float delta, void* stream_) {
    HRN_CHECK(residual && shifts && beta_prev && beta && weighted, -2, "hrn_robust_apply: null argument");
    unsigned tx, ty;
    if (!robust_shape("hrn_robust_apply", B, V, H, W, scale, &tx, &ty) || !delta_ok("hrn_robust_apply", delta)) return -2;
    const size_t lr = (size_t)B * V * H * W * 4, sh = (size_t)B * V * 8;
    HRN_CHECK(!overlaps(weighted, lr, residual, lr) && !(lr_masks && overlaps(weighted, lr, lr_masks, lr)) && !overlaps(weighted, lr, shifts, sh) &&
                  !(alphas && overlaps(weighted, lr, alphas, sh / 2)) && !overlaps(weighted, lr, beta_prev, sh / 2) &&
                  !overlaps(weighted, lr, beta, sh / 2),
              -2, "hrn_robust_apply: weighted must not alias an input (it is a second plane)");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("robust_apply", 0.0, (double)lr * (lr_masks ? 3 : 2), stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((robust_kernel<decltype(s)::value, true>), grid, block, 0, stream, residual, lr_masks, alphas, shifts, beta_prev, beta,
                           weighted, (double*)nullptr, delta, tiles, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_btv_step(const float* x, const float* c, float* out, int planes, int SH, int SW, int P, float alpha, float eps,
                            void* stream) {
    return btv_map<BTV_STEP>("hrn_btv_step", x, c, out, planes, SH, SW, P, alpha, eps, stream);
}

extern "C" int hrn_btv_backward(const float* x, const float* gain, float* out, int planes, int SH, int SW, int P, float alpha, float eps,
                                void* stream) {
    return btv_map<BTV_BACKWARD>("hrn_btv_backward", x, gain, out, planes, SH, SW, P, alpha, eps, stream);
}

extern "C" size_t hrn_btv_workspace_bytes(int planes, int SH, int SW) {
    if (!(planes > 0 && SH > 0 && SW > 0) || SH > kBtvMaxSide || SW > kBtvMaxSide) return 0;
    return btv_bytes(planes, SH, SW);
}

extern "C" int hrn_btv_value(const float* x, float* value, void* workspace, size_t workspace_bytes, int planes, int SH, int SW, int P,
                             float alpha, float eps, float gain, void* stream_) {
    HRN_CHECK(x && value && workspace, -2, "hrn_btv_value: null argument");
    unsigned tx, ty;
    BtvWeights wt;
    if (!btv_shape("hrn_btv_value", planes, SH, SW, P, alpha, eps, &tx, &ty, &wt)) return -2;
    HRN_CHECK(std::isfinite(gain), -2, "hrn_btv_value: gain must be finite (got %g)", (double)gain);
    const size_t need = btv_bytes(planes, SH, SW), bytes = (size_t)planes * SH * SW * 4;
    HRN_CHECK(workspace_bytes >= need, -2, "hrn_btv_value: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    HRN_CHECK(((uintptr_t)workspace & 7u) == 0, -2, "hrn_btv_value: workspace must be 8-byte aligned");
    HRN_CHECK(!overlaps(workspace, need, x, bytes) && !overlaps(value, (size_t)planes * 4, x, bytes) &&
                  !overlaps(value, (size_t)planes * 4, workspace, need),
              -2, "hrn_btv_value: value, workspace and x must not alias each other");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t per_plane = (size_t)tx * ty, tiles = per_plane * (size_t)planes;
    HrnProfScope prof("btv_value", 0.0, (double)bytes + 2.0 * (double)need, stream);
    btv_launch<BTV_VALUE>(P, x, nullptr, nullptr, (double*)workspace, wt, eps, tiles, SH, SW, tx, ty, stream);
    HRN_LAUNCH_CHECK();
    hipLaunchKernelGGL(btv_value_finish_kernel, dim3((unsigned)planes), dim3(kThreads), 0, stream, (const double*)workspace, value, per_plane,
                       (double)SH * (double)SW, gain);
    HRN_LAUNCH_CHECK();
    return 0;
}
