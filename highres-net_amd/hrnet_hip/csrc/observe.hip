// The observation model of multi-frame super-resolution and its adjoint (hrn_observe, hrn_consistency_residual, hrn_consistency_finish,
// hrn_observe_adjoint; the definition is in include/hrnet_hip.h).  (No counterpart in the reference.)
//
// Along an axis, sample i of a view shifted by dy reads the S + 5 HR rows S i + n - 2 + j, j = 0 .. S + 4, with ONE weight vector w_j per
// view and axis: c = -S dy (fp64, rounded to fp32, clamped as split_and_taps of mncc_common.h clamps), n = floor(c), f = c - n, and
// w_j = (1 / S) sum_k t_{j - 2 - k}(f) over the S point samples k of the LR pixel's box, t the six normalised taps of the 7f sampler.  The
// taps are the formula of split_and_taps kept in fp64 (that function rounds each tap to fp32; the definition rounds once, after the box
// sum): one (view, axis, tap) per thread into LDS, then one (view, axis, j) per thread.
//
// The tile, its walk, the test whether a view counts and the list of a chunk's views are lr_tile.h's, shared with upsample.hip and
// shift_add.hip.
//
// Forward / residual: a workgroup of 256 threads owns TH x TW = 8 x 32 samples of ONE view.
//   1. win[8 S + 5][S][PW]  <- the HR window whose origin follows (n_y, n_x), DE-INTERLEAVED by column phase (column u -> plane u mod S,
//      index u div S), zero outside the frame; 16-byte global loads where a row allows (its address 16-byte aligned, chosen per row; the
//      chunks that cross the frame's edge element by element), all of a thread's loads issued before its first LDS write
//   2. hrow[8 S + 5][32]    <- the row pass: sum_j wx_j win[r][S x + j], a lane per LR column: tap j reads plane j mod S at x + j div S, a
//      UNIT-stride ds_read_b32 (banks are the address mod 32 within a half-wave: no conflict; interleaved it would be stride S, 2-way at
//      x2 and 4-way at x4)
//   3. a thread per sample: sum_j wy_j hrow[S y + j][x], unit stride again; valid, counted, the output, and in the residual form the
//      tile's fp64 partials of n, sum e, sum e^2 (lanes by xor exchanges, the four waves in order: a fixed order)
//   The staging writes are not conflict-free (word k of 32 consecutive chunks is stride 4 in u, and a half-wave straddles two window
//   rows): 3.6 / 3.1 / 1.9-way on average at x2 / x3 / x4, counted from the addresses.
// Finish: one workgroup per sample; a wave per view adds that view's tile partials (a lane every 64th tile in index order, then the lanes
//   by xor exchanges), and thread 0 adds the views in index order.  Everything stays in device memory.
// Adjoint: a workgroup owns the S TH x S TW HR pixels of 8 x 32 LR cells of one sample and walks the views in index order, in chunks of
//   kChunk whose weights it forms first.  HR row Y receives from view row i with the weight w_j, j = Y + 2 - n - S i: with
//   2 - n = S e + q (0 <= q < S, uniform per view) the pixel S m + p of the tile reads the rows y0 + e + m + mr - a, a = 0 .. (S + 4) / S,
//   mr = (p + q) div S, with j = (p + q) mod S + S a: for a compile-time q every index is a constant, so the S variants are chosen by a
//   uniform switch and no register is indexed by a run-time value.  Per view:
//   1. rs[TH + 1 + AM][TW + 1 + AM]  <- [counted] (residual + beta_v), counted re-derived from frame, shift, mask (the next view's loads
//      are in flight during passes 2 and 3)
//   2. tv[S TH][TW + 1 + AM]         <- the gather along y of every staged column
//   3. G[S][S] in registers          += the gather along x of tv
//   then out = coef G, or x - coef G (x may be out: a thread reads what it writes).  One writer per element, no atomics.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are stated in DESIGN.md section 7t.
#include "observe_geom.h"

#include <cmath>

namespace {

constexpr int kChunk = 32;                               // views whose weights a workgroup of the adjoint forms at a time
static_assert(kChunk <= 64, "compact_chunk takes a chunk in one wave");
constexpr int kFinishThreads = 1024;

// (hr_coord, split64, view_in_reach and sample_valid are observe_geom.h's, shared with robust_sr.hip; plane_stride, tap64, box_weight and
// floor_div are there too, shared with observe_shift.hip)

// ----------------------------------------------------------------------------- forward / residual
// RESIDUAL false: views = A x where valid, valid 0 / 1.  true: residual = e where counted, and the tile's partials.
template <int S, bool RESIDUAL>
__global__ __launch_bounds__(kThreads) void observe_kernel(const float* __restrict__ hr, const float* __restrict__ lrs,
                                                           const float* __restrict__ masks, const float* __restrict__ alphas,
                                                           const float* __restrict__ shifts, float* __restrict__ out, float* __restrict__ valid,
                                                           double* __restrict__ partials, size_t tiles, int V, int H, int W, unsigned tiles_x,
                                                           unsigned tiles_y) {
    constexpr int NW = S + 5, WH = kTH * S + 5, WW = kTW * S + 5, PW = plane_stride(S);
    constexpr int NC = (WW + 3 + 3) / 4;                 // 16-byte chunks that cover a window row from any alignment
    constexpr int LPT = (WH * NC + kThreads - 1) / kThreads, RPT = (WH * kTW + kThreads - 1) / kThreads;
    static_assert((WW - 1) / S < PW, "a plane holds its share of a window row");
    __shared__ float win[WH][S][PW];
    __shared__ float hrow[WH][kTW];
    __shared__ double k6[2][6];
    __shared__ float wl[2][NW];
    __shared__ int nn[2];
    __shared__ double red[kThreads / 64][3];
    const int SH = S * H, SW = S * W, tid = threadIdx.x, ty = tid / kTW, tx = tid - ty * kTW;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);         // tp.n: the view's plane, b V + v
        const int iy = tp.y0 + ty, ix = tp.x0 + tx;
        const bool inside = iy < H && ix < W;
        const size_t at = tp.n * (size_t)H * W + (size_t)(inside ? iy : 0) * W + (inside ? ix : 0);
        const bool counts = view_counts(RESIDUAL ? alphas : nullptr, shifts, tp.n) && view_in_reach<S>(shifts, tp.n);     // uniform
        if (!counts) {
            if (inside) {
                out[at] = 0.f;
                if (!RESIDUAL) valid[at] = 0.f;
            }
            if (RESIDUAL && tid < 3) partials[3 * tile + tid] = 0.0;
            continue;
        }
        // the sample's own view value and mask: in flight during the staging
        float yv = 0.f, mv = 1.f;
        if (RESIDUAL && inside) {
            yv = lrs[at];
            if (masks) mv = masks[at];
        }
        if (tid < 12) {
            const int ax = tid / 6, o = tid - 6 * ax;
            int n;
            double f;
            split64(hr_coord(S, shifts[2 * tp.n + ax]), &n, &f);
            k6[ax][o] = tap64(o - 2, f);
            if (o == 0) nn[ax] = n;
        }
        __syncthreads();                                             // also: the previous tile's reads of win / hrow / wl / red are done
        if (tid < 2 * NW) {
            const int ax = tid / NW, j = tid - NW * ax;
            wl[ax][j] = box_weight<S>(k6[ax], j);
        }
        const int ny = nn[0], nx = nn[1];
        const int uy0 = S * tp.y0 + ny - 2, ux0 = S * tp.x0 + nx - 2;      // the window's origin on the HR grid
        const int a0 = floor_div(ux0, 4) * 4;                              // the first chunk's column
        const float* plane = hr + (tp.n / (size_t)V) * (size_t)SH * SW;
        f32x4 ld[LPT];
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int e = tid + i * kThreads, r = e / NC, c = e - r * NC;
            const int gy = uy0 + r, gx = a0 + 4 * c;
            ld[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < WH * NC && gy >= 0 && gy < SH && gx + 3 >= 0 && gx < SW) {
                const float* row = plane + (size_t)gy * SW;
                if (gx >= 0 && gx + 4 <= SW && ((uintptr_t)row & 15u) == 0) ld[i] = *(const f32x4*)(row + gx);
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (gx + k >= 0 && gx + k < SW) ld[i][k] = row[gx + k];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int e = tid + i * kThreads, r = e / NC, c = e - r * NC;
            if (e < WH * NC) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int u = a0 + 4 * c + k - ux0;              // 0 .. WW - 1 inside the window
                    if (u >= 0 && u < WW) win[r][u % S][u / S] = ld[i][k];
                }
            }
        }
        __syncthreads();
        float w[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = wl[1][j];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int e = tid + i * kThreads, r = e / kTW, x = e - r * kTW;
            if (e < WH * kTW) {
                float s = w[0] * win[r][0][x];
#pragma unroll
                for (int j = 1; j < NW; ++j) s = fmaf(w[j], win[r][j % S][x + j / S], s);
                hrow[r][x] = s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = wl[0][j];
        float s = w[0] * hrow[S * ty][tx];
#pragma unroll
        for (int j = 1; j < NW; ++j) s = fmaf(w[j], hrow[S * ty + j][tx], s);
        const bool ok = inside && sample_valid<S>(iy, ny, H) && sample_valid<S>(ix, nx, W);
        if (!RESIDUAL) {
            if (inside) {
                out[at] = ok ? s : 0.f;
                valid[at] = ok ? 1.f : 0.f;
            }
        } else {
            const bool counted = ok && mv != 0.f;
            const float e = counted ? s - yv : 0.f;
            if (inside) out[at] = e;
            double v0 = counted ? 1.0 : 0.0, v1 = (double)e, v2 = (double)e * (double)e;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                v0 += __shfl_xor(v0, m);
                v1 += __shfl_xor(v1, m);
                v2 += __shfl_xor(v2, m);
            }
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

// ----------------------------------------------------------------------------- finish
// stats of a sample out of the tiles' partials; block b = sample b, a wave per view, kFinishThreads / 64 views a round
__global__ __launch_bounds__(kFinishThreads) void consistency_finish_kernel(const double* __restrict__ partials, float* __restrict__ beta,
                                                                           int* __restrict__ count, double* __restrict__ ssr,
                                                                           float* __restrict__ loss, int* __restrict__ n_views,
                                                                           float* __restrict__ coef_loss, float* __restrict__ coef_step, int V,
                                                                           size_t per_view, int scale, float step, int brightness) {
    constexpr int WAVES = kFinishThreads / 64;
    __shared__ double round_q[WAVES], round_n[WAVES];
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0, q_all = 0.0;                     // thread 0's: the views in index order
    int nv = 0;
    for (int v0 = 0; v0 < V; v0 += WAVES) {
        const int v = v0 + wave;
        if (v < V) {
            const size_t bv = b * (size_t)V + (size_t)v;
            const double* p = partials + 3 * bv * per_view;
            double n = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4
            for (size_t t = lane; t < per_view; t += 64) { n += p[3 * t]; s1 += p[3 * t + 1]; s2 += p[3 * t + 2]; }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                n += __shfl_xor(n, m);
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (lane == 0) {
                // sum (e + beta)^2 over the counted pixels with the beta that is stored (fp32): s2 + 2 beta s1 + n beta^2
                const float bt = brightness && n > 0.0 ? (float)(-s1 / n) : 0.f;
                const double bf = (double)bt, q = s2 + 2.0 * bf * s1 + n * bf * bf;
                beta[bv] = bt;
                count[bv] = (int)n;
                ssr[bv] = round_q[wave] = q > 0.0 ? q : 0.0;
                round_n[wave] = n;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < WAVES && v0 + w < V; ++w) { total += round_n[w]; q_all += round_q[w]; nv += round_n[w] > 0.0; }
        __syncthreads();                                 // the round's sums are taken before the next round writes them
    }
    if (threadIdx.x == 0) {
        loss[b] = total > 0.0 ? (float)(q_all / total) : 0.f;
        n_views[b] = nv;
        coef_loss[b] = total > 0.0 ? (float)(2.0 / total) : 0.f;
        coef_step[b] = nv > 0 ? (float)((double)step * (double)(scale * scale) / (double)nv) : 0.f;
    }
}

// ----------------------------------------------------------------------------- adjoint
// out[p] = sum_a w[(p + Q) mod S + S a] in[(p + Q) div S + AM - a] for the S pixels p of a cell: rows ascending (a descending)
template <int S, int Q>
__device__ __forceinline__ void gather_axis(const float* w, const float* in, float* out) {
    constexpr int AM = (S + 4) / S;
#pragma unroll
    for (int p = 0; p < S; ++p) {
        const int ph = (p + Q) % S, mr = (p + Q) / S;
        float acc = 0.f;
#pragma unroll
        for (int a = AM; a >= 0; --a)
            if (ph + S * a <= S + 4) acc = fmaf(w[ph + S * a], in[mr + AM - a], acc);
        out[p] = acc;
    }
}

template <int S>
__device__ __forceinline__ void gather_q(int q, const float* w, const float* in, float* out) {
    switch (q) {                                         // uniform: q belongs to the view
        case 0: gather_axis<S, 0>(w, in, out); break;
        case 1: gather_axis<S, 1>(w, in, out); break;
        case 2: if (S > 2) gather_axis<S, (S > 2 ? 2 : 0)>(w, in, out); break;
        default: if (S > 3) gather_axis<S, (S > 3 ? 3 : 0)>(w, in, out); break;
    }
}

// x and out may be the same pointer (no __restrict__ on either)
template <int S>
__global__ __launch_bounds__(kThreads) void observe_adjoint_kernel(const float* __restrict__ res, const float* __restrict__ masks,
                                                                   const float* __restrict__ alphas, const float* __restrict__ shifts,
                                                                   const float* __restrict__ beta, const float* __restrict__ coef,
                                                                   const float* __restrict__ gain, const float* x, float* out, size_t tiles,
                                                                   int V, int H, int W, unsigned tiles_x, unsigned tiles_y) {
    constexpr int NW = S + 5, AM = (S + 4) / S, RH = kTH + 1 + AM, RW = kTW + 1 + AM, TR = S * kTH;
    constexpr int LPT = (RH * RW + kThreads - 1) / kThreads;
    __shared__ float rs[RH][RW];
    __shared__ float tv[TR][RW];
    __shared__ double k6[kChunk][2][6];
    __shared__ float wl[kChunk][2][NW];
    __shared__ int nn[kChunk][2];
    __shared__ int list[kChunk], n_list;                 // the views of the chunk that count and are in reach, in index order
    const int SH = S * H, SW = S * W, tid = threadIdx.x, ty = tid / kTW, tx = tid - ty * kTW;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);         // tp.n: the sample
        float G[S][S];
#pragma unroll
        for (int p = 0; p < S; ++p)
#pragma unroll
            for (int r = 0; r < S; ++r) G[p][r] = 0.f;
        for (int v0 = 0; v0 < V; v0 += kChunk) {
            const int nv = min(kChunk, V - v0);
            __syncthreads();                             // the previous chunk's (or tile's) last reads of k6 / wl / nn / list are done
            for (int e = tid; e < nv * 12; e += kThreads) {
                const int vi = e / 12, ax = (e / 6) % 2, o = e % 6;
                int n;
                double f;
                split64(hr_coord(S, shifts[2 * (tp.n * (size_t)V + (size_t)(v0 + vi)) + ax]), &n, &f);
                k6[vi][ax][o] = tap64(o - 2, f);
                if (o == 0) nn[vi][ax] = n;
            }
            if (tid < 64) {                              // the first wave compacts the chunk's views (kChunk <= 64)
                const size_t bv = tp.n * (size_t)V + (size_t)(v0 + min(tid, nv - 1));
                compact_chunk(tid < nv && view_counts(alphas, shifts, bv) && view_in_reach<S>(shifts, bv), list, &n_list);
            }
            __syncthreads();
            for (int e = tid; e < nv * 2 * NW; e += kThreads) {
                const int vi = e / (2 * NW), ax = (e / NW) % 2, j = e % NW;
                wl[vi][ax][j] = box_weight<S>(k6[vi][ax], j);
            }
            __syncthreads();
            float pr[LPT];
            auto fetch = [&](int vi) {                   // [counted] (residual + beta) of the view's window
                const size_t bv = tp.n * (size_t)V + (size_t)(v0 + vi);
                const int ny = nn[vi][0], nx = nn[vi][1];
                const int wy0 = tp.y0 + floor_div(2 - ny, S) - AM, wx0 = tp.x0 + floor_div(2 - nx, S) - AM;
                const float bt = beta ? beta[bv] : 0.f;
#pragma unroll
                for (int i = 0; i < LPT; ++i) {
                    const int e = tid + i * kThreads, r = e / RW, c = e - r * RW;
                    const int gy = wy0 + r, gx = wx0 + c;
                    const bool in = e < RH * RW && sample_valid<S>(gy, ny, H) && sample_valid<S>(gx, nx, W);
                    const size_t at = bv * (size_t)H * W + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
                    const float rv = in ? res[at] : 0.f;
                    const float mk = in && masks ? masks[at] : 1.f;
                    pr[i] = in && mk != 0.f ? rv + bt : 0.f;
                }
            };
            const int nl = n_list;
            if (nl > 0) fetch(list[0]);
            for (int li = 0; li < nl; ++li) {
                const int vi = list[li];
#pragma unroll
                for (int i = 0; i < LPT; ++i) {
                    const int e = tid + i * kThreads, r = e / RW, c = e - r * RW;
                    if (e < RH * RW) rs[r][c] = pr[i];
                }
                __syncthreads();                         // also: every thread is past the previous view's reads of tv
                if (li + 1 < nl) fetch(list[li + 1]);
                const int ny = nn[vi][0], nx = nn[vi][1];
                const int qy = 2 - ny - S * floor_div(2 - ny, S), qx = 2 - nx - S * floor_div(2 - nx, S);
                float w[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) w[j] = wl[vi][0][j];
                for (int e = tid; e < kTH * RW; e += kThreads) {
                    const int yy = e / RW, c = e - yy * RW;
                    float in[AM + 2], o[S];
#pragma unroll
                    for (int k = 0; k < AM + 2; ++k) in[k] = rs[yy + k][c];
                    gather_q<S>(qy, w, in, o);
#pragma unroll
                    for (int p = 0; p < S; ++p) tv[S * yy + p][c] = o[p];
                }
                __syncthreads();                         // also: the next view's rs is not written before this
#pragma unroll
                for (int j = 0; j < NW; ++j) w[j] = wl[vi][1][j];
#pragma unroll
                for (int p = 0; p < S; ++p) {
                    float in[AM + 2], o[S];
#pragma unroll
                    for (int k = 0; k < AM + 2; ++k) in[k] = tv[S * ty + p][tx + k];
                    gather_q<S>(qx, w, in, o);
#pragma unroll
                    for (int r = 0; r < S; ++r) G[p][r] += o[r];
                }
            }
        }
        const int iy = tp.y0 + ty, ix = tp.x0 + tx;
        if (iy < H && ix < W) {
            const float cf = (coef ? coef[tp.n] : 1.f) * (gain ? gain[tp.n] : 1.f);
#pragma unroll
            for (int p = 0; p < S; ++p) {
                const size_t at = (tp.n * (size_t)SH + (size_t)(S * iy + p)) * (size_t)SW + (size_t)S * ix;
                float xv[S];
#pragma unroll
                for (int r = 0; r < S; ++r) xv[r] = x ? x[at + r] : 0.f;
#pragma unroll
                for (int r = 0; r < S; ++r) out[at + r] = x ? fmaf(-cf, G[p][r], xv[r]) : cf * G[p][r];
            }
        }
    }
}

// what every entry point refuses; -> true, or false with the error set
bool check_shape(const char* fn, int B, int V, int H, int W, int scale, unsigned* tiles_x, unsigned* tiles_y) {
    *tiles_x = *tiles_y = 0;
    if (!(B > 0 && V > 0 && H > 0 && W > 0)) { hrn_set_error("%s: empty input B=%d V=%d H=%d W=%d", fn, B, V, H, W); return false; }
    if (!check_side_scale(fn, "frames", H, W, scale)) return false;
    // 2^60 elements (upsample.hip and shift_add.hip stop at 2^62; no reason for the difference is recorded)
    if ((size_t)B > ((size_t)1 << 60) / ((size_t)V * scale * scale * H * W)) {
        hrn_set_error("%s: %d x %d frames of %d x %d exceed the address space", fn, B, V, H, W);
        return false;
    }
    plane_tiles(H, W, tiles_x, tiles_y);
    return true;
}

// three fp64 partials per tile of every view
size_t workspace_bytes(int B, int V, int H, int W) { return (size_t)B * V * plane_tiles(H, W) * 3 * sizeof(double); }

}  // namespace

extern "C" size_t hrn_observe_workspace_bytes(int B, int V, int H, int W) {
    if (!(B > 0 && V > 0 && H > 0 && W > 0) || H > kMaxSide || W > kMaxSide) return 0;
    return workspace_bytes(B, V, H, W);
}

extern "C" int hrn_observe(const float* hr, const float* shifts, float* views, float* valid, int B, int V, int H, int W, int scale,
                           void* stream_) {
    HRN_CHECK(hr && shifts && views && valid, -2, "hrn_observe: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_observe", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t lr = (size_t)B * V * H * W * 4, sr = (size_t)B * H * W * scale * scale * 4, sh = (size_t)B * V * 8;
    HRN_CHECK(!overlaps(views, lr, valid, lr) && !overlaps(views, lr, hr, sr) && !overlaps(valid, lr, hr, sr) && !overlaps(views, lr, shifts, sh) &&
                  !overlaps(valid, lr, shifts, sh),
              -2, "hrn_observe: views and valid must not alias each other or an input");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("observe", 0.0, (double)sr + 2.0 * (double)lr, stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((observe_kernel<decltype(s)::value, false>), grid, block, 0, stream, hr, (const float*)nullptr, (const float*)nullptr,
                           (const float*)nullptr, shifts, views, valid, (double*)nullptr, tiles, V, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_consistency_residual(const float* hr, const float* lrs, const float* lr_masks, const float* alphas, const float* shifts,
                                        float* residual, void* workspace, size_t workspace_bytes_, int B, int V, int H, int W, int scale,
                                        void* stream_) {
    HRN_CHECK(hr && lrs && shifts && residual && workspace, -2, "hrn_consistency_residual: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_consistency_residual", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t need = workspace_bytes(B, V, H, W);
    HRN_CHECK(workspace_bytes_ >= need, -2, "hrn_consistency_residual: workspace of %zu bytes, %zu needed", workspace_bytes_, need);
    HRN_CHECK(((uintptr_t)workspace & 7u) == 0, -2, "hrn_consistency_residual: workspace must be 8-byte aligned");
    const size_t lr = (size_t)B * V * H * W * 4, sr = (size_t)B * H * W * scale * scale * 4, sh = (size_t)B * V * 8;
    HRN_CHECK(!overlaps(residual, lr, hr, sr) && !overlaps(residual, lr, lrs, lr) && !(lr_masks && overlaps(residual, lr, lr_masks, lr)) &&
                  !overlaps(residual, lr, shifts, sh) && !(alphas && overlaps(residual, lr, alphas, sh / 2)) && !overlaps(residual, lr, workspace, need),
              -2, "hrn_consistency_residual: residual must not alias another argument");
    HRN_CHECK(!overlaps(workspace, need, hr, sr) && !overlaps(workspace, need, lrs, lr) && !(lr_masks && overlaps(workspace, need, lr_masks, lr)) &&
                  !overlaps(workspace, need, shifts, sh) && !(alphas && overlaps(workspace, need, alphas, sh / 2)),
              -2, "hrn_consistency_residual: workspace must not alias an input");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("consistency_residual", 0.0, (double)sr + (double)lr * (lr_masks ? 3 : 2) + (double)need, stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((observe_kernel<decltype(s)::value, true>), grid, block, 0, stream, hr, lrs, lr_masks, alphas, shifts, residual,
                           (float*)nullptr, (double*)workspace, tiles, V, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_consistency_finish(const void* workspace, size_t workspace_bytes_, float* beta, int* count, void* ssr, float* loss,
                                      int* n_views, float* coef_loss, float* coef_step, int B, int V, int H, int W, int scale, float step,
                                      int brightness, void* stream_) {
    HRN_CHECK(workspace && beta && count && ssr && loss && n_views && coef_loss && coef_step, -2, "hrn_consistency_finish: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_consistency_finish", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t need = workspace_bytes(B, V, H, W);
    HRN_CHECK(workspace_bytes_ >= need, -2, "hrn_consistency_finish: workspace of %zu bytes, %zu needed", workspace_bytes_, need);
    HRN_CHECK(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)ssr & 7u) == 0, -2, "hrn_consistency_finish: workspace and ssr must be 8-byte aligned");
    HRN_CHECK(std::isfinite(step) && step > 0.f && step < 2.f, -2, "hrn_consistency_finish: step must lie in (0, 2) (got %g)", (double)step);
    const size_t bv = (size_t)B * V;
    const void* outs[7] = {beta, count, ssr, loss, n_views, coef_loss, coef_step};
    const size_t bytes[7] = {bv * 4, bv * 4, bv * 8, (size_t)B * 4, (size_t)B * 4, (size_t)B * 4, (size_t)B * 4};
    for (int i = 0; i < 7; ++i) {
        HRN_CHECK(!overlaps(outs[i], bytes[i], workspace, need), -2, "hrn_consistency_finish: an output must not alias the workspace");
        for (int j = i + 1; j < 7; ++j)
            HRN_CHECK(!overlaps(outs[i], bytes[i], outs[j], bytes[j]), -2, "hrn_consistency_finish: the outputs must not alias each other");
    }
    hipStream_t stream = (hipStream_t)stream_;
    HrnProfScope prof("consistency_finish", 0.0, (double)need, stream);
    hipLaunchKernelGGL(consistency_finish_kernel, dim3((unsigned)B), dim3(kFinishThreads), 0, stream, (const double*)workspace, beta, count,
                       (double*)ssr, loss, n_views, coef_loss, coef_step, V, (size_t)tx * ty, scale, step, brightness ? 1 : 0);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_observe_adjoint(const float* residual, const float* lr_masks, const float* alphas, const float* shifts, const float* beta,
                                   const float* coef, const float* gain, const float* x, float* out, int B, int V, int H, int W, int scale,
                                   void* stream_) {
    HRN_CHECK(residual && shifts && out, -2, "hrn_observe_adjoint: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_observe_adjoint", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t lr = (size_t)B * V * H * W * 4, sr = (size_t)B * H * W * scale * scale * 4, sh = (size_t)B * V * 8;
    HRN_CHECK(!overlaps(out, sr, residual, lr) && !(lr_masks && overlaps(out, sr, lr_masks, lr)) && !overlaps(out, sr, shifts, sh) &&
                  !(alphas && overlaps(out, sr, alphas, sh / 2)) && !(beta && overlaps(out, sr, beta, sh / 2)) &&
                  !(coef && overlaps(out, sr, coef, (size_t)B * 4)) && !(gain && overlaps(out, sr, gain, (size_t)B * 4)),
              -2, "hrn_observe_adjoint: out must not alias an input (only x may be out itself)");
    HRN_CHECK(!x || x == out || !overlaps(x, sr, out, sr), -2, "hrn_observe_adjoint: x must be out itself or apart from it");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B;
    HrnProfScope prof("observe_adjoint", 0.0, (double)lr * (lr_masks ? 2 : 1) + (double)sr * (x ? 2 : 1), stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL(observe_adjoint_kernel<decltype(s)::value>, grid, block, 0, stream, residual, lr_masks, alphas, shifts, beta, coef, gain,
                           x, out, tiles, V, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}
