// The shift-searched cMSE / cPSNR as a differentiable training tail:
//   shift_cPSNR(sr, hr, hr_map, border_w)   reference src/Evaluator.py:52-73   (the search over the integer offsets of hr)
//   get_loss(srs, hrs, hr_maps, metric)     reference src/train.py:66-87       (the per-offset brightness-corrected cMSE)
// With beta = border, h = H - 2 beta, w = W - 2 beta, s = the centre crop of sr, and for the offset k = u (2 beta + 1) + v
//   g = hr[u:u+h, v:v+w], m = map[u:u+h, v:v+w], d = s - g, S0 = sum m, S1 = sum m d, S2 = sum m d^2:
//   n_k = S0, bias_k = -S1 / S0, cMSE_k = (S2 - S1^2 / S0) / S0        (one pass, three fp64 sums: losses.hip)
// and k* = the lowest k of minimal cMSE_k among the offsets with n_k > 0.  The gradient goes through k* alone:
//   d out / d sr[beta + y, beta + x] = c m*[y, x] (s[y, x] + bias* - g*[y, x]),  c = 2 / n*  or  -20 / (ln 10 n* cMSE*)
//
// Forward, stage 1: a workgroup owns a 32 x 128 tile of one sample's centre crop (for w <= 128 that is a band of crop rows).  It
// stages that tile of hr and map plus the 2 beta halo rows and columns in LDS once, keeps its 16 sr pixels per thread in registers and
// walks the (2 beta + 1)^2 offsets out of LDS: for a row offset u a lane reads the 4 + 2 beta floats under its four pixels as 16-byte
// reads and takes every column offset v from those registers, so no shifted copy of a row is ever read from LDS.  A wave's 16-lane
// read groups lie inside one tile row, on 16 different 16-byte slots: conflict-free at any row stride.  Every pixel of the three
// images comes from HBM once (the halo re-reads of neighbouring tiles hit L2): 12 B H W bytes.  Stage 2 adds the tiles' sums in a
// fixed order (runs of tiles in parallel, the runs in order) and picks k*.  No floating-point atomics: the result is bit-reproducible.
#include "kernels.h"
#include "wave_sums.h"

namespace {

constexpr int SL_TW = 128;          // tile width: 32 lanes x 4 pixels
constexpr int SL_RPT = 4;           // crop rows per thread (2 measured: 6 % faster at 192 x 192, 11 % slower at 384 x 384)
constexpr int SL_TH = 8 * SL_RPT;   // tile height: 8 thread rows x SL_RPT
constexpr int SL_MAX_BORDER = 8;

// grid (tiles, B).  partial [B][tiles][(2 beta + 1)^2][3] = {S0, S1, S2} of the tile at every offset.
template <int BETA>
__global__ __launch_bounds__(256) void shift_loss_partial_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                                 const float* __restrict__ maps, int H, int W, int clip, int ntx,
                                                                 double* __restrict__ partial) {
    constexpr int NB = 2 * BETA + 1;
    constexpr int NQ = (4 + 2 * BETA + 3) / 4;          // 16-byte reads that cover a lane's 4 + 2 beta floats
    constexpr int STRIDE = SL_TW - 4 + 4 * NQ;          // the last lane's span ends the row; a multiple of 4 floats
    constexpr int ROWS = SL_TH + 2 * BETA;
    constexpr int NV = 3 * NB, P = pow2_ceil(NV);
    __shared__ __attribute__((aligned(16))) float lg[ROWS * STRIDE];
    __shared__ __attribute__((aligned(16))) float lm[ROWS * STRIDE];
    __shared__ double red[4][P];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = tid & 31, ly = tid >> 5;
    const int tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * SL_TH, x0 = tx * SL_TW;         // the tile's origin: crop coordinates == hr coordinates at offset (0, 0)
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
    float s[SL_RPT][4];
    unsigned valid = 0;
#pragma unroll
    for (int r = 0; r < SL_RPT; ++r)
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

    double* out = partial + ((size_t)blockIdx.y * gridDim.x + tile) * (NB * NB * 3);
#pragma unroll 1
    for (int u = 0; u < NB; ++u) {
        double a[P];
#pragma unroll
        for (int i = 0; i < P; ++i) a[i] = 0.0;
#pragma unroll
        for (int r = 0; r < SL_RPT; ++r) {
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
                for (int v = 0; v < NB; ++v) {
                    const double mm = (double)m[j + v];
                    const double d = sd - (double)g[j + v];
                    const double md = mm * d;
                    a[3 * v] += mm;
                    a[3 * v + 1] += md;
                    a[3 * v + 2] = fma(md, d, a[3 * v + 2]);
                }
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

// grid (B), 1024 threads.  Adds the tiles in a fixed order - the tiles are cut into as many runs as fit the workgroup, a thread adds one
// run of one sum with eight loads in flight, the runs are added in order - then takes the lowest k of minimal cMSE_k among n_k > 0.
constexpr int SL_FIN_THREADS = 1024;
__global__ __launch_bounds__(SL_FIN_THREADS) void shift_loss_finish_kernel(const double* __restrict__ partial, int ntiles, int nk, int metric,
                                                                           float* __restrict__ out, double* __restrict__ stats) {
    constexpr int MAXK = (2 * SL_MAX_BORDER + 1) * (2 * SL_MAX_BORDER + 1);
    __shared__ double acc[SL_FIN_THREADS];
    __shared__ double cn[MAXK], cb[MAXK], cm[MAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nv = 3 * nk;                               // <= 867
    int runs = SL_FIN_THREADS / nv;
    if (runs > ntiles) runs = ntiles;
    const int per = (ntiles + runs - 1) / runs;
    const double* p = partial + (size_t)b * ntiles * nv;
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
    __syncthreads();
    for (int k = tid; k < nk; k += SL_FIN_THREADS) {
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

// grid (rows of blocks, B): one elementwise pass over all of d_srs, the border frame and clamped pixels written as zeros.
__global__ __launch_bounds__(256) void shift_loss_backward_kernel(const float* __restrict__ srs, const float* __restrict__ hrs,
                                                                  const float* __restrict__ maps, const double* __restrict__ stats,
                                                                  const float* __restrict__ d_out, int H, int W, int border, int metric,
                                                                  int clip, float* __restrict__ d_srs) {
    const int b = blockIdx.y;
    const double cnt = stats[4 * b + 0], bias = stats[4 * b + 1], cmse = stats[4 * b + 2];
    const int k = (int)stats[4 * b + 3];
    const int nb = 2 * border + 1;
    const bool none = !(cnt > 0.0) || k < 0 || k >= nb * nb;     // no clear pixel (or stats of another border): zeros, nothing read out of bounds
    const int u = none ? 0 : k / nb, v = none ? 0 : k - (k / nb) * nb;
    // d out / d cMSE: cMSE itself -> 1;  -10 log10(cMSE) -> -10 / (ln 10 cMSE)
    const double dm = metric == 1 ? 1.0 : -10.0 / (2.302585092994046 * cmse);
    const float coef = none ? 0.f : (float)((double)d_out[b] * dm * 2.0 / cnt);
    const float fb = (float)bias;
    const size_t n = (size_t)H * W, base = (size_t)b * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int Y = (int)(i / W), X = (int)(i - (size_t)Y * W);
        float grad = 0.f;
        if (!none && Y >= border && Y < H - border && X >= border && X < W - border) {
            const float s = srs[base + i];
            if (!clip || (s >= 0.f && s <= 1.f)) {       // torch.clamp passes the gradient on [min, max], ends included
                const size_t j = base + (size_t)(Y - border + u) * W + (X - border + v);
                grad = coef * maps[j] * (s - hrs[j] + fb);
            }
        }
        d_srs[base + i] = grad;
    }
}

template <int BETA>
void launch_partial(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int clip, int ntx, int ntiles,
                    double* partial, hipStream_t stream) {
    hipLaunchKernelGGL(shift_loss_partial_kernel<BETA>, dim3(ntiles, B), dim3(256), 0, stream, srs, hrs, maps, H, W, clip, ntx, partial);
}

size_t tiles_of(int H, int W, int border, int* ntx) {
    const int h = H - 2 * border, w = W - 2 * border;
    const int nx = (w + SL_TW - 1) / SL_TW, ny = (h + SL_TH - 1) / SL_TH;
    if (ntx) *ntx = nx;
    return (size_t)nx * ny;
}

}  // namespace

size_t hrn_shift_loss_workspace_bytes_impl(int B, int H, int W, int border) {
    const size_t nk = (size_t)(2 * border + 1) * (2 * border + 1);
    return (size_t)B * tiles_of(H, W, border, nullptr) * nk * 3 * sizeof(double);
}

int hrn_launch_shift_loss_train(const float* srs, const float* hrs, const float* maps, int B, int H, int W, int border, int metric,
                                int clip, float* out, double* stats, double* partial, hipStream_t stream) {
    HRN_CHECK(border >= 0 && border <= SL_MAX_BORDER, -2, "shift loss: border %d outside 0..%d", border, SL_MAX_BORDER);
    int ntx = 0;
    const size_t tiles = tiles_of(H, W, border, &ntx);
    HRN_CHECK(tiles <= 0x7fffffffu, -2, "shift loss: %zu tiles exceed the grid limit", tiles);
    const int ntiles = (int)tiles;
    HrnProfScope prof("shift_loss_fwd", 0.0, 12.0 * B * H * W, stream);
    switch (border) {
        case 0: launch_partial<0>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 1: launch_partial<1>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 2: launch_partial<2>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 3: launch_partial<3>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 4: launch_partial<4>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 5: launch_partial<5>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 6: launch_partial<6>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        case 7: launch_partial<7>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
        default: launch_partial<8>(srs, hrs, maps, B, H, W, clip, ntx, ntiles, partial, stream); break;
    }
    HRN_LAUNCH_CHECK();
    const int nk = (2 * border + 1) * (2 * border + 1);
    hipLaunchKernelGGL(shift_loss_finish_kernel, dim3(B), dim3(SL_FIN_THREADS), 0, stream, (const double*)partial, ntiles, nk, metric, out, stats);
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
