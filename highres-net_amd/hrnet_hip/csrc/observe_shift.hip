// The observation model's derivative in the shifts (hrn_observe_shift_grad / _grad_finish, hrn_shift_normal / _normal_finish; the
// definition is in include/hrnet_hip.h).  (No counterpart in the reference.)
//
// With c = -S d per axis, w_j = (1 / S) sum_k t_{j-2-k}(f) is observe.hip's weight vector and omega_j = dw_j / dd = -sum_k k'_{j-2-k}(f)
// its derivative, k' the derivative tap of the six-tap sampler (section 7p: k'_o = (u'_o - k_o sum u') / sum u, the series for sinc'
// below |t| = 1e-2), both formed in fp64 and rounded to fp32 once.  For a valid sample the derivative images are
// D_y = (omega^y (x) w^x) x and D_x = (w^y (x) omega^x) x on the (S + 5)^2 footprint of A x.
//
// Tile kernel: observe_kernel's geometry - 256 threads own 8 x 32 samples of ONE view, the HR window staged once and de-interleaved by
// column phase - with two row passes (w^x and omega^x, sharing their LDS reads) and three column passes, so that a thread holds A x, D_y
// and D_x of its sample.  A x is observe_kernel's expression, operation for operation: the residual it writes has that kernel's bits.
//   GRAD:   v = counted ? g + beta_v : 0 (a select), the tile's fp64 sums of v D_y and v D_x.
//   NORMAL: e = A x - y where counted, p = counted (plain) or robust_sr.hip's Welsch weight of e + beta_prev, and the tile's ten fp64 sums
//           p, p e, p e^2, p D_y, p D_x, p e D_y, p e D_x, p D_y^2, p D_y D_x, p D_x^2 (products in fp64 of the fp32 values).
//           On request also observe_kernel<S, true>'s three plain sums n, sum e, sum e^2 in its layout and with its bits (in plain mode
//           the first three of the ten; in Welsch mode a reduction of their own), for hrn_consistency_finish to run on unchanged.
//   Lanes by xor exchanges, the four waves in order: a fixed order, no atomics.
// Finish kernels: a wave per view adds that view's tile sums (a lane every 64th tile in index order, then the lanes by xor exchanges).
//   Grad: d_shifts = fp32(coef gain sum).  Normal: the centred normal equations in fp64 from the uncentred sums, and the damped
//   Gauss-Newton update of the shift into a second buffer.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage) are stated in DESIGN.md section 7v.
#include "observe_geom.h"

#include <cmath>

namespace {

constexpr int kSums = HRN_SHIFT_NORMAL_SUMS;             // doubles per tile in the workspace (the grad mode uses the first two)
constexpr int kFinishThreads = 256;
constexpr double kMinWeight = 3.0;                       // a view whose sum p is below this keeps its shift

// sinc(t) = sin(pi t) / (pi t) as tap64 forms it, and its derivative with section 7p's series below 1e-2
__device__ __forceinline__ void sinc_slope64(double t, double* s, double* ds) {
    const double z = 3.141592653589793 * t;
    *s = t == 0.0 ? 1.0 : sin(z) / z;
    *ds = fabs(t) < 1e-2 ? 3.141592653589793 * z * (-1.0 / 3.0 + z * z * (1.0 / 30.0 - z * z / 840.0)) : (cos(z) - *s) / t;
}

// u'_o = d/df of the raw tap o (-2 .. 3), fp64
__device__ __forceinline__ double dtap64(int o, double f) {
    const double x = (double)o - f;
    double a, da, b, db;
    sinc_slope64(x, &a, &da);
    sinc_slope64(x / 3.0, &b, &db);
    return fabs(x) >= 3.0 ? 0.0 : -(da * b + a * db / 3.0);
}

// omega_j out of the raw taps k[0..5] and their derivatives dk[0..5]: -sum_s k'_{j-s}, rounded once
template <int S>
__device__ __forceinline__ float box_slope(const double* k, const double* dk, int j) {
    double sum = 0.0, dsum = 0.0;
#pragma unroll
    for (int o = 0; o < 6; ++o) { sum += k[o]; dsum += dk[o]; }
    double w = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int o = j - s;
        if (o >= 0 && o < 6) w += (dk[o] - (k[o] / sum) * dsum) / sum;
    }
    return (float)(-w);
}

// robust_sr.hip's weight: fp32 sum, quotient, square, expf
__device__ __forceinline__ float welsch_weight(bool counted, float e, float bp, float delta) {
    const float u = (e + bp) / delta;
    return counted ? expf(-(u * u)) : 0.f;
}

// ----------------------------------------------------------------------------- the tile kernel
// NORMAL false: g = the incoming gradient plane, masks / alphas / beta optional.  true: lrs, masks / alphas / beta_prev optional, the
// residual plane optional, and `plain` optional: observe_kernel<S, true>'s three sums per tile, in its layout and with its bits.
template <int S, bool NORMAL>
__global__ __launch_bounds__(kThreads) void observe_shift_kernel(const float* __restrict__ hr, const float* __restrict__ in,
                                                                 const float* __restrict__ masks, const float* __restrict__ alphas,
                                                                 const float* __restrict__ shifts, const float* __restrict__ beta, float delta,
                                                                 float* __restrict__ residual, double* __restrict__ partials,
                                                                 double* __restrict__ plain, size_t tiles, int V, int H, int W,
                                                                 unsigned tiles_x, unsigned tiles_y) {
    constexpr int NW = S + 5, WH = kTH * S + 5, WW = kTW * S + 5, PW = plane_stride(S);
    constexpr int NC = (WW + 3 + 3) / 4;                 // 16-byte chunks that cover a window row from any alignment
    constexpr int LPT = (WH * NC + kThreads - 1) / kThreads, RPT = (WH * kTW + kThreads - 1) / kThreads;
    constexpr int NS = NORMAL ? kSums : 2;
    static_assert((WW - 1) / S < PW, "a plane holds its share of a window row");
    __shared__ float win[WH][S][PW];
    __shared__ float hrow[2][WH][kTW];                   // the row pass with w^x, and with omega^x
    __shared__ double k6[2][6], dk6[2][6];
    __shared__ float wl[2][2][NW];                       // [w, omega][axis][j]
    __shared__ int nn[2];
    __shared__ double red[kThreads / 64][NS];
    const int SH = S * H, SW = S * W, tid = threadIdx.x, ty = tid / kTW, tx = tid - ty * kTW;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const TilePos tp = tile_pos(tile, tiles_x, tiles_y);         // tp.n: the view's plane, b V + v
        const int iy = tp.y0 + ty, ix = tp.x0 + tx;
        const bool inside = iy < H && ix < W;
        const size_t at = tp.n * (size_t)H * W + (size_t)(inside ? iy : 0) * W + (inside ? ix : 0);
        const bool counts = view_counts(alphas, shifts, tp.n) && view_in_reach<S>(shifts, tp.n);     // uniform
        if (!counts) {
            if (NORMAL && residual && inside) residual[at] = 0.f;
            if (tid < NS) partials[kSums * tile + tid] = 0.0;
            if (NORMAL && plain && tid < 3) plain[3 * tile + tid] = 0.0;
            continue;
        }
        // the sample's own plane value and mask: in flight during the staging
        float yv = 0.f, mv = 1.f;
        if (inside) {
            yv = in[at];
            if (masks) mv = masks[at];
        }
        const float bt = beta ? beta[tp.n] : 0.f;
        if (tid < 12) {
            const int ax = tid / 6, o = tid - 6 * ax;
            int n;
            double f;
            split64(hr_coord(S, shifts[2 * tp.n + ax]), &n, &f);
            k6[ax][o] = tap64(o - 2, f);
            dk6[ax][o] = dtap64(o - 2, f);
            if (o == 0) nn[ax] = n;
        }
        __syncthreads();                                             // also: the previous tile's reads of win / hrow / wl / red are done
        if (tid < 2 * NW) {
            const int ax = tid / NW, j = tid - NW * ax;
            wl[0][ax][j] = box_weight<S>(k6[ax], j);
            wl[1][ax][j] = box_slope<S>(k6[ax], dk6[ax], j);
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
        float w[NW], om[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) { w[j] = wl[0][1][j]; om[j] = wl[1][1][j]; }
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int e = tid + i * kThreads, r = e / kTW, x = e - r * kTW;
            if (e < WH * kTW) {
                const float v0 = win[r][0][x];
                float s = w[0] * v0, d = om[0] * v0;
#pragma unroll
                for (int j = 1; j < NW; ++j) {
                    const float v = win[r][j % S][x + j / S];
                    s = fmaf(w[j], v, s);
                    d = fmaf(om[j], v, d);
                }
                hrow[0][r][x] = s;
                hrow[1][r][x] = d;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NW; ++j) { w[j] = wl[0][0][j]; om[j] = wl[1][0][j]; }
        float s, dy, dx;
        {
            const float h0 = hrow[0][S * ty][tx];
            s = w[0] * h0;
            dy = om[0] * h0;
            dx = w[0] * hrow[1][S * ty][tx];
        }
#pragma unroll
        for (int j = 1; j < NW; ++j) {
            const float h = hrow[0][S * ty + j][tx];
            s = fmaf(w[j], h, s);
            dy = fmaf(om[j], h, dy);
            dx = fmaf(w[j], hrow[1][S * ty + j][tx], dx);
        }
        const bool counted = inside && sample_valid<S>(iy, ny, H) && sample_valid<S>(ix, nx, W) && mv != 0.f;
        double v[NS], u[3] = {0.0, 0.0, 0.0};             // u: observe_kernel's plain sums n, sum e, sum e^2, for `plain` in Welsch mode
        if (!NORMAL) {
            const double g = counted ? (double)(yv + bt) : 0.0;
            v[0] = counted ? g * (double)dy : 0.0;
            v[1] = counted ? g * (double)dx : 0.0;
        } else {
            const float e = counted ? s - yv : 0.f;
            if (residual && inside) residual[at] = e;
            const float pw = beta ? welsch_weight(counted, e, bt, delta) : (counted ? 1.f : 0.f);
            const double p = (double)pw, ed = (double)e, yd = counted ? (double)dy : 0.0, xd = counted ? (double)dx : 0.0;
            v[0] = p;
            v[1] = p * ed;
            v[2] = p * ed * ed;
            v[3] = p * yd;
            v[4] = p * xd;
            v[5] = p * ed * yd;
            v[6] = p * ed * xd;
            v[7] = p * yd * yd;
            v[8] = p * yd * xd;
            v[9] = p * xd * xd;
            u[0] = counted ? 1.0 : 0.0;
            u[1] = ed;
            u[2] = ed * ed;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
            for (int q = 0; q < NS; ++q) v[q] += __shfl_xor(v[q], m);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < NS; ++q) red[tid / 64][q] = v[q];
        }
        __syncthreads();
        if (tid < NS) {
            double t = red[0][tid];
#pragma unroll
            for (int wv = 1; wv < kThreads / 64; ++wv) t += red[wv][tid];
            partials[kSums * tile + tid] = t;
            if (NORMAL && plain && !beta && tid < 3) plain[3 * tile + tid] = t;      // plain mode: p = counted, the first three ARE them
        }
        if (NORMAL && plain && beta) {                   // uniform: the three plain sums by a reduction of their own, observe_kernel's order
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
                for (int q = 0; q < 3; ++q) u[q] += __shfl_xor(u[q], m);
            }
            __syncthreads();                             // the reads of red above are done
            if ((tid & 63) == 0) {
#pragma unroll
                for (int q = 0; q < 3; ++q) red[tid / 64][q] = u[q];
            }
            __syncthreads();
            if (tid < 3) {
                double t = red[0][tid];
#pragma unroll
                for (int wv = 1; wv < kThreads / 64; ++wv) t += red[wv][tid];
                plain[3 * tile + tid] = t;
            }
        }
    }
}

// ----------------------------------------------------------------------------- finish
// a view's tile sums: a lane every 64th tile in index order, then the lanes by xor exchanges; every lane returns the totals
template <int N>
__device__ __forceinline__ void view_sums(const double* __restrict__ p, size_t per_view, int lane, double* t) {
#pragma unroll
    for (int q = 0; q < N; ++q) t[q] = 0.0;
    for (size_t i = lane; i < per_view; i += 64) {
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] += p[kSums * i + q];
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int q = 0; q < N; ++q) t[q] += __shfl_xor(t[q], m);
    }
}

// d_shifts[bv][a] = fp32(coef[b] gain[b] sum_a); a wave per view
__global__ __launch_bounds__(kFinishThreads) void shift_grad_finish_kernel(const double* __restrict__ partials, const float* __restrict__ coef,
                                                                          const float* __restrict__ gain, float* __restrict__ d_shifts,
                                                                          size_t views, int V, size_t per_view) {
    const int lane = threadIdx.x & 63;
    const size_t bv = (size_t)blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (bv >= views) return;
    double t[2];
    view_sums<2>(partials + kSums * bv * per_view, per_view, lane, t);
    if (lane < 2) {
        const size_t b = bv / (size_t)V;
        const double cf = (coef ? (double)coef[b] : 1.0) * (gain ? (double)gain[b] : 1.0);
        d_shifts[2 * bv + lane] = (float)(cf * (lane ? t[1] : t[0]));
    }
}

// normal[bv][0..7] and, with shifts_out, the damped Gauss-Newton update; a wave per view
template <int S>
__global__ __launch_bounds__(kFinishThreads) void shift_normal_finish_kernel(const double* __restrict__ partials, const float* __restrict__ alphas,
                                                                            const float* __restrict__ shifts,
                                                                            const unsigned char* __restrict__ fixed, double* __restrict__ normal,
                                                                            float* __restrict__ shifts_out, size_t views, size_t per_view,
                                                                            int brightness, double damping, double max_step) {
    const int lane = threadIdx.x & 63;
    const size_t bv = (size_t)blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (bv >= views) return;
    double t[kSums];
    view_sums<kSums>(partials + kSums * bv * per_view, per_view, lane, t);
    if (lane != 0) return;
    const double P = t[0], Se = t[1], See = t[2], Sy = t[3], Sx = t[4], Sey = t[5], Sex = t[6], Syy = t[7], Syx = t[8], Sxx = t[9];
    const bool live = P >= 0x1p-60;
    const double bt = brightness && live ? -Se / P : 0.0;
    const double my = brightness && live ? Sy / P : 0.0, mx = brightness && live ? Sx / P : 0.0;
    const double rest = Se + bt * P;                     // sum p (e + beta): 0 with brightness up to its rounding
    const double gy = Sey + bt * Sy - my * rest, gx = Sex + bt * Sx - mx * rest;
    const double Hyy = Syy - my * Sy, Hyx = Syx - my * Sx, Hxx = Sxx - mx * Sx;
    const double q = See + 2.0 * bt * Se + bt * bt * P;
    double* o = normal + 8 * bv;
    o[0] = P; o[1] = gy; o[2] = gx; o[3] = Hyy; o[4] = Hyx; o[5] = Hxx; o[6] = bt; o[7] = q > 0.0 ? q : 0.0;
    if (!shifts_out) return;
    const float d0 = shifts[2 * bv], d1 = shifts[2 * bv + 1];
    float n0 = d0, n1 = d1;                              // a view that keeps its shift keeps its bits (a NaN's too: no arithmetic)
    const bool counts = view_counts(alphas, shifts, bv) && view_in_reach<S>(shifts, bv);
    if (counts && !(fixed && fixed[bv]) && P >= kMinWeight) {
        const double lam = damping * (Hyy + Hxx) * 0.5, a = Hyy + lam, d = Hxx + lam, det = a * d - Hyx * Hyx;
        if (det > 0.0 && isfinite(det)) {
            double sy = -(d * gy - Hyx * gx) / det, sx = -(a * gx - Hyx * gy) / det;
            const double m = fmax(fabs(sy), fabs(sx));
            if (m > max_step) { sy *= max_step / m; sx *= max_step / m; }
            if (isfinite(sy) && isfinite(sx)) {
                n0 = (float)((double)d0 + sy);
                n1 = (float)((double)d1 + sx);
            }
        }
    }
    // bit copies where kept: through integers, so that a signalling NaN is not quieted on the way
    unsigned* out = (unsigned*)shifts_out + 2 * bv;
    out[0] = __float_as_uint(n0);
    out[1] = __float_as_uint(n1);
}

// what every entry point refuses; -> true, or false with the error set
bool check_shape(const char* fn, int B, int V, int H, int W, int scale, unsigned* tiles_x, unsigned* tiles_y) {
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

size_t workspace_bytes(int B, int V, int H, int W) { return (size_t)B * V * plane_tiles(H, W) * kSums * sizeof(double); }

bool check_workspace(const char* fn, const void* workspace, size_t given, size_t need) {
    if (given < need) { hrn_set_error("%s: workspace of %zu bytes, %zu needed", fn, given, need); return false; }
    if (((uintptr_t)workspace & 7u) != 0) { hrn_set_error("%s: workspace must be 8-byte aligned", fn); return false; }
    return true;
}

// `out` (nout bytes) against the listed inputs (null entries skipped)
bool apart(const void* out, size_t nout, const void* const* ins, const size_t* bytes, int n) {
    for (int i = 0; i < n; ++i)
        if (ins[i] && overlaps(out, nout, ins[i], bytes[i])) return false;
    return true;
}

}  // namespace

extern "C" size_t hrn_observe_shift_workspace_bytes(int B, int V, int H, int W) {
    if (!(B > 0 && V > 0 && H > 0 && W > 0) || H > kMaxSide || W > kMaxSide) return 0;
    return workspace_bytes(B, V, H, W);
}

extern "C" int hrn_observe_shift_grad(const float* hr, const float* g, const float* lr_masks, const float* alphas, const float* shifts,
                                      const float* beta, void* workspace, size_t workspace_bytes_, int B, int V, int H, int W, int scale,
                                      void* stream_) {
    HRN_CHECK(hr && g && shifts && workspace, -2, "hrn_observe_shift_grad: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_observe_shift_grad", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t need = workspace_bytes(B, V, H, W);
    if (!check_workspace("hrn_observe_shift_grad", workspace, workspace_bytes_, need)) return -2;
    const size_t lr = (size_t)B * V * H * W * 4, sr = (size_t)B * H * W * scale * scale * 4, sh = (size_t)B * V * 8;
    const void* ins[6] = {hr, g, lr_masks, alphas, shifts, beta};
    const size_t bytes[6] = {sr, lr, lr, sh / 2, sh, sh / 2};
    HRN_CHECK(apart(workspace, need, ins, bytes, 6), -2, "hrn_observe_shift_grad: workspace must not alias an input");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("observe_shift_grad", 0.0, (double)sr + (double)lr * (lr_masks ? 2 : 1) + (double)need, stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((observe_shift_kernel<decltype(s)::value, false>), grid, block, 0, stream, hr, g, lr_masks, alphas, shifts, beta, 0.f,
                           (float*)nullptr, (double*)workspace, (double*)nullptr, tiles, V, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_observe_shift_grad_finish(const void* workspace, size_t workspace_bytes_, const float* coef, const float* gain,
                                             float* d_shifts, int B, int V, int H, int W, void* stream_) {
    HRN_CHECK(workspace && d_shifts, -2, "hrn_observe_shift_grad_finish: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_observe_shift_grad_finish", B, V, H, W, 2, &tx, &ty)) return -2;
    const size_t need = workspace_bytes(B, V, H, W);
    if (!check_workspace("hrn_observe_shift_grad_finish", workspace, workspace_bytes_, need)) return -2;
    const size_t sh = (size_t)B * V * 8;
    const void* ins[3] = {workspace, coef, gain};
    const size_t bytes[3] = {need, (size_t)B * 4, (size_t)B * 4};
    HRN_CHECK(apart(d_shifts, sh, ins, bytes, 3), -2, "hrn_observe_shift_grad_finish: d_shifts must not alias an input");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t views = (size_t)B * V;
    HrnProfScope prof("observe_shift_grad_finish", 0.0, (double)need, stream);
    hipLaunchKernelGGL(shift_grad_finish_kernel, dim3((unsigned)((views + 3) / 4)), dim3(kFinishThreads), 0, stream, (const double*)workspace,
                       coef, gain, d_shifts, views, V, (size_t)tx * ty);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_shift_normal(const float* hr, const float* lrs, const float* lr_masks, const float* alphas, const float* shifts,
                                const float* beta_prev, float delta, float* residual, void* plain_workspace, size_t plain_bytes,
                                void* workspace, size_t workspace_bytes_, int B, int V, int H, int W, int scale, void* stream_) {
    HRN_CHECK(hr && lrs && shifts && workspace, -2, "hrn_shift_normal: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_shift_normal", B, V, H, W, scale, &tx, &ty)) return -2;
    HRN_CHECK(!beta_prev || (std::isfinite(delta) && delta > 0.f), -2, "hrn_shift_normal: delta must be positive (got %g)", (double)delta);
    const size_t need = workspace_bytes(B, V, H, W);
    if (!check_workspace("hrn_shift_normal", workspace, workspace_bytes_, need)) return -2;
    const size_t lr = (size_t)B * V * H * W * 4, sr = (size_t)B * H * W * scale * scale * 4, sh = (size_t)B * V * 8;
    const void* ins[7] = {hr, lrs, lr_masks, alphas, shifts, beta_prev, residual};
    const size_t bytes[7] = {sr, lr, lr, sh / 2, sh, sh / 2, lr};
    HRN_CHECK(apart(workspace, need, ins, bytes, 7), -2, "hrn_shift_normal: workspace must not alias another argument");
    HRN_CHECK(!residual || apart(residual, lr, ins, bytes, 6), -2, "hrn_shift_normal: residual must not alias an input");
    const size_t plain_need = need / kSums * 3;          // hrn_observe_workspace_bytes: three fp64 sums per tile
    if (plain_workspace) {
        if (!check_workspace("hrn_shift_normal (plain_workspace)", plain_workspace, plain_bytes, plain_need)) return -2;
        HRN_CHECK(apart(plain_workspace, plain_need, ins, bytes, 7) && !overlaps(plain_workspace, plain_need, workspace, need), -2,
                  "hrn_shift_normal: plain_workspace must not alias another argument");
    }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t tiles = (size_t)tx * ty * (size_t)B * (size_t)V;
    HrnProfScope prof("shift_normal", 0.0, (double)sr + (double)lr * ((lr_masks ? 2 : 1) + (residual ? 1 : 0)) + (double)need, stream);
    const dim3 grid(blocks_for(tiles)), block(kThreads);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL((observe_shift_kernel<decltype(s)::value, true>), grid, block, 0, stream, hr, lrs, lr_masks, alphas, shifts, beta_prev,
                           beta_prev ? delta : 1.f, residual, (double*)workspace, (double*)plain_workspace, tiles, V, H, W, tx, ty);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_shift_normal_finish(const void* workspace, size_t workspace_bytes_, const float* alphas, const float* shifts,
                                       const unsigned char* fixed, void* normal, float* shifts_out, int B, int V, int H, int W, int scale,
                                       int brightness, float damping, float max_step, void* stream_) {
    HRN_CHECK(workspace && shifts && normal, -2, "hrn_shift_normal_finish: null argument");
    unsigned tx, ty;
    if (!check_shape("hrn_shift_normal_finish", B, V, H, W, scale, &tx, &ty)) return -2;
    const size_t need = workspace_bytes(B, V, H, W);
    if (!check_workspace("hrn_shift_normal_finish", workspace, workspace_bytes_, need)) return -2;
    HRN_CHECK(((uintptr_t)normal & 7u) == 0, -2, "hrn_shift_normal_finish: normal must be 8-byte aligned");
    if (shifts_out) {
        HRN_CHECK(std::isfinite(damping) && damping >= 0.f, -2, "hrn_shift_normal_finish: damping must be finite and >= 0 (got %g)", (double)damping);
        HRN_CHECK(std::isfinite(max_step) && max_step > 0.f, -2, "hrn_shift_normal_finish: max_step must be finite and positive (got %g)",
                  (double)max_step);
    }
    const size_t views = (size_t)B * V, sh = views * 8, nb = views * 64;
    const void* ins[4] = {workspace, alphas, shifts, fixed};
    const size_t bytes[4] = {need, sh / 2, sh, views};
    HRN_CHECK(apart(normal, nb, ins, bytes, 4), -2, "hrn_shift_normal_finish: normal must not alias an input");
    HRN_CHECK(!shifts_out || (apart(shifts_out, sh, ins, bytes, 4) && !overlaps(shifts_out, sh, normal, nb)), -2,
              "hrn_shift_normal_finish: shifts_out must not alias shifts or another argument");
    hipStream_t stream = (hipStream_t)stream_;
    HrnProfScope prof("shift_normal_finish", 0.0, (double)need, stream);
    hrn_by_scale(scale, [&](auto s) {
        hipLaunchKernelGGL(shift_normal_finish_kernel<decltype(s)::value>, dim3((unsigned)((views + 3) / 4)), dim3(kFinishThreads), 0, stream,
                           (const double*)workspace, alphas, shifts, fixed, (double*)normal, shifts_out, views, (size_t)tx * ty,
                           brightness ? 1 : 0, (double)damping, (double)max_step);
    });
    HRN_LAUNCH_CHECK();
    return 0;
}
