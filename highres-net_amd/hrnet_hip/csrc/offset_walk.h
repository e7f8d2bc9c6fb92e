// What the shift-searched losses share (shift_loss.hip, cl1_loss.hip): the walk of one tile over every integer offset of hr, the
// fixed-order sum of a sample's tiles, the frame of the backward pass and the border dispatch.  A loss supplies its terms.
//
// The walk: a workgroup owns a 32 x 128 tile of one sample's centre crop (for w <= 128 that is a band of crop rows).  It stages that
// tile of hr and map plus the 2 beta halo rows and columns in LDS once, keeps its 16 sr pixels per thread in registers and walks the
// (2 beta + 1)^2 offsets out of LDS: for a row offset u a lane reads the 4 + 2 beta floats under its four pixels as 16-byte reads and
// takes every column offset v from those registers, so no shifted copy of a row is ever read from LDS.  A wave's 16-lane read groups
// lie inside one tile row, on 16 different 16-byte slots: conflict-free at any row stride.  No floating-point atomics anywhere: every
// sum has a fixed order, so a result is bit-reproducible and a sample's does not depend on its batch.
#pragma once
#include <type_traits>
#include "kernels.h"
#include "wave_sums.h"

namespace {

constexpr int OW_TW = 128;          // tile width: 32 lanes x 4 pixels
constexpr int OW_RPT = 4;           // crop rows per thread (2 measured: 6 % faster at 192 x 192, 11 % slower at 384 x 384)
constexpr int OW_TH = 8 * OW_RPT;   // tile height: 8 thread rows x OW_RPT
constexpr int OW_MAX_BORDER = 8;
constexpr int OW_MAXK = (2 * OW_MAX_BORDER + 1) * (2 * OW_MAX_BORDER + 1);
constexpr int OW_FIN_THREADS = 1024;        // the workgroup of a kernel that calls sum_tile_runs

inline size_t tiles_of(int H, int W, int border, int* ntx) {
    const int h = H - 2 * border, w = W - 2 * border;
    const int nx = (w + OW_TW - 1) / OW_TW, ny = (h + OW_TH - 1) / OW_TH;
    if (ntx) *ntx = nx;
    return (size_t)nx * ny;
}

inline size_t nk_of(int border) { return (size_t)(2 * border + 1) * (2 * border + 1); }

// f(std::integral_constant<int, border>) for a border of 0..OW_MAX_BORDER, which the caller has checked.
template <class F>
void with_border(int border, F&& f) {
    switch (border) {
        case 0: f(std::integral_constant<int, 0>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

// The body of a kernel with grid (tiles, B) and 256 threads.  partial [B][tiles][(2 beta + 1)^2][Term::SUMS]: the tile's sums at every
// offset.  A Term has
//   SUMS                                   the number of sums per offset
//   row<NB>(u)                             what it needs once per row of offsets, uniform over the workgroup
//   add(row, v, m, s, g, a)                adds one pixel at the offset (u, v) - map m, sr s, hr g, in fp64 - into its SUMS sums a
template <int BETA, class Term>
__device__ __forceinline__ void offset_walk(const float* __restrict__ srs, const float* __restrict__ hrs, const float* __restrict__ maps,
                                            int H, int W, int clip, int ntx, const Term& term, double* __restrict__ partial) {
    constexpr int NB = 2 * BETA + 1;
    constexpr int NQ = (4 + 2 * BETA + 3) / 4;          // 16-byte reads that cover a lane's 4 + 2 beta floats
    constexpr int STRIDE = OW_TW - 4 + 4 * NQ;          // the last lane's span ends the row; a multiple of 4 floats
    constexpr int ROWS = OW_TH + 2 * BETA;
    constexpr int NS = Term::SUMS, NV = NS * NB, P = pow2_ceil(NV);
    __shared__ __attribute__((aligned(16))) float lg[ROWS * STRIDE];
    __shared__ __attribute__((aligned(16))) float lm[ROWS * STRIDE];
    __shared__ double red[4][P];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = tid & 31, ly = tid >> 5;
    const int tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * OW_TH, x0 = tx * OW_TW;         // the tile's origin: crop coordinates == hr coordinates at offset (0, 0)
    const int h = H - 2 * BETA, w = W - 2 * BETA;
    const size_t img = (size_t)blockIdx.y * H * W;
    const float* sr = srs + img;
    const float* hr = hrs + img;
    const float* mp = maps + img;

    // staging, eight rounds of loads in flight before the first LDS write: a workgroup has one wave per SIMD, so nothing else hides
    // the latency of a load
    constexpr int NST = ROWS * STRIDE, DEPTH = 8;
    for (int i0 = tid; i0 < NST; i0 += 256 * DEPTH) {
        float gv[DEPTH], mv[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const int i = i0 + 256 * k;
            const int rr = i / STRIDE, cc = i - rr * STRIDE;
            const int Y = y0 + rr, X = x0 + cc;
            const bool in = i < NST && Y < H && X < W;
            const size_t j = (size_t)Y * W + X;
            gv[k] = in ? hr[j] : 0.f;
            mv[k] = in ? mp[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const int i = i0 + 256 * k;
            if (i < NST) { lg[i] = gv[k]; lm[i] = mv[k]; }
        }
    }
    float s[OW_RPT][4];
    unsigned valid = 0;
#pragma unroll
    for (int r = 0; r < OW_RPT; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = y0 + ly + 8 * r, x = x0 + 4 * lx + j;
            const bool in = y < h && x < w;
            float t = in ? sr[(size_t)(y + BETA) * W + (x + BETA)] : 0.f;
            if (clip) t = t != t ? t : fminf(fmaxf(t, 0.f), 1.f);       // torch.clamp keeps NaN; fminf / fmaxf alone turn it into 0
            s[r][j] = t;
            valid |= (unsigned)in << (4 * r + j);
        }
    __syncthreads();

    double* out = partial + ((size_t)blockIdx.y * gridDim.x + tile) * (NB * NB * NS);
#pragma unroll 1
    for (int u = 0; u < NB; ++u) {
        const auto row = term.template row<NB>(u);
        double a[P];
#pragma unroll
        for (int i = 0; i < P; ++i) a[i] = 0.0;
#pragma unroll
        for (int r = 0; r < OW_RPT; ++r) {
            const int base = (ly + 8 * r + u) * STRIDE + 4 * lx;
            float g[4 * NQ], m[4 * NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                f32x4 gv = *reinterpret_cast<const f32x4*>(&lg[base + 4 * q]);
                f32x4 mv = *reinterpret_cast<const f32x4*>(&lm[base + 4 * q]);
                asm volatile("" : "+v"(gv), "+v"(mv));      // keep the reads whole (ds_read_b128): unused lanes would split them
                g[4 * q] = gv.x; g[4 * q + 1] = gv.y; g[4 * q + 2] = gv.z; g[4 * q + 3] = gv.w;
                m[4 * q] = mv.x; m[4 * q + 1] = mv.y; m[4 * q + 2] = mv.z; m[4 * q + 3] = mv.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((valid >> (4 * r + j)) & 1)) continue;
                const double sd = (double)s[r][j];
#pragma unroll
                for (int v = 0; v < NB; ++v) term.add(row, v, (double)m[j + v], sd, (double)g[j + v], &a[NS * v]);
            }
        }
        WaveSums<P, 0>::run(a, lane);
        const int idx = wave_sums_index<P>(lane);
        __syncthreads();                                 // the previous offset row's readers of `red` are done
        if (lane < P) red[wave][idx] = a[0];
        __syncthreads();
        if (tid < NV) out[u * NV + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// Adds a sample's tiles in a fixed order, in a workgroup of OW_FIN_THREADS: the tiles are cut into as many runs as fit the workgroup, a
// thread adds one run of one sum with eight loads in flight into acc[run * nv + value].  p [ntiles][nv], nv <= OW_FIN_THREADS.
// -> the number of runs, which the caller adds in order after a barrier.
__device__ __forceinline__ int sum_tile_runs(const double* __restrict__ p, int ntiles, int nv, double* acc) {
    const int tid = threadIdx.x;
    int runs = OW_FIN_THREADS / nv;
    if (runs > ntiles) runs = ntiles;
    const int per = (ntiles + runs - 1) / runs;
    if (tid < runs * nv) {
        const int run = tid / nv, val = tid - run * nv;
        const int t0 = run * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
        double sum = 0.0;
        int t = t0;
        for (; t + 8 <= t1; t += 8) {
            double x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = p[(size_t)(t + q) * nv + val];
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += x[q];
        }
        for (; t < t1; ++t) sum += p[(size_t)t * nv + val];
        acc[tid] = sum;
    }
    return runs;
}

// The body of a backward kernel with grid (rows of blocks, B): one elementwise pass over all of d_srs, the border frame and clamped
// pixels written as zeros.  stats [B][NSTAT] = {n*, b*, value*, k*, ...}.  make(the sample's stats row, none) -> grad(s, g, m), the
// gradient at a pixel of the crop from sr there and from hr and map at the selected offset; none: the sample has no gradient.
// `block` is a default argument so that blockDim.x is read in the kernel itself: only there does the compiler know the workgroups to be
// uniform and take it from the kernel's arguments with one scalar load, without the test for a partial last workgroup.
template <int NSTAT, class Make>
__device__ __forceinline__ void offset_walk_backward(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                     const float* __restrict__ maps, const double* __restrict__ stats, int H, int W,
                                                     int border, int clip, float* __restrict__ d_srs, Make make,
                                                     unsigned block = blockDim.x) {
    const int b = blockIdx.y;
    double st[NSTAT];                                    // the whole row first: one load, ahead of every branch
#pragma unroll
    for (int j = 0; j < NSTAT; ++j) st[j] = stats[NSTAT * b + j];
    const int k = (int)st[3];
    const int nb = 2 * border + 1;
    const bool none = !(st[0] > 0.0) || k < 0 || k >= nb * nb;   // no clear pixel (or stats of another border): zeros, nothing read out of bounds
    const int u = none ? 0 : k / nb, v = none ? 0 : k - (k / nb) * nb;
    const auto grad_of = make(st, none);
    const size_t n = (size_t)H * W, base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * block + threadIdx.x; i < n; i += (size_t)gridDim.x * block) {
        const int Y = (int)(i / W), X = (int)(i - (size_t)Y * W);
        float grad = 0.f;
        if (!none && Y >= border && Y < H - border && X >= border && X < W - border) {
            const float s = srs[base + i];
            if (!clip || (s >= 0.f && s <= 1.f)) {       // torch.clamp passes the gradient on [min, max], ends included
                const size_t j = base + (size_t)(Y - border + u) * W + (X - border + v);
                grad = grad_of(s, hrs[j], maps[j]);
            }
        }
        d_srs[base + i] = grad;
    }
}

}  // namespace
