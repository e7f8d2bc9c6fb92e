// What the masked-NCC registration paths share (DESIGN.md sections 7f, 7g and 7i): registration.hip, a view resident in one CU's LDS, and
// registration_scene.hip / registration_local.hip, frames of any size in tiles.  The split of a coordinate into whole pixels, fraction
// and six taps, the bilinear mask test and its table, a grid coordinate, the six taps down a run, a thread's sums over a run and their
// way to the workgroup's totals, the score out of the six sums, the first-maximum rule and the host's rule of the levels are written once,
// so that the paths cannot drift apart.  Everything is in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_sums.h"

#pragma clang fp contract(off)      // every fused multiply-add of both paths is written out: kernels that share a level must round alike

namespace {

constexpr int RG_NSUM = 6;                      // n, sum t, sum r, sum t^2, sum r^2, sum r t
constexpr int RG_RUN = 8;                       // rows of one column that a thread takes at a time, in every path
constexpr float RG_DMAX = 256.f;                // a coordinate beyond this leaves no pixel valid (the scene path: see its halo)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// d -> n = floor(d), f = d - n (exact in fp64) and the six normalised taps k_o = sinc(o - f) sinc((o - f) / 3), o = -2..3
__device__ void split_and_taps(float d, int* n, double* f, float* tap) {
    const float dc = fminf(fmaxf(d, -RG_DMAX), RG_DMAX);        // also takes a NaN to a finite value; beyond +-RG_DMAX nothing is valid anyway
    const double fl = floor((double)dc);
    const double fr = (double)dc - fl;
    double k[6], sum = 0.0;
#pragma unroll
    for (int o = 0; o < 6; ++o) {
        const double x = (double)(o - 2) - fr;
        const double px = 3.141592653589793 * x, px3 = 3.141592653589793 * (x / 3.0);
        const double a = x == 0.0 ? 1.0 : sin(px) / px;
        const double b = x == 0.0 ? 1.0 : sin(px3) / px3;
        k[o] = fabs(x) >= 3.0 ? 0.0 : a * b;
        sum += k[o];
    }
#pragma unroll
    for (int o = 0; o < 6; ++o) tap[o] = (float)(k[o] / sum);
    *n = (int)fl;
    *f = fr;
}

// (1 - fy) ((1 - fx) q0 + fx q1) + fy ((1 - fx) q2 + fx q3) > 0.5: the bilinear sample of the mask at (y, x), (y, x + 1), (y + 1, x),
// (y + 1, x + 1) = q0..q3.  fp64, in the order the definition writes it.
__device__ __forceinline__ bool mask_sample(double fy, double fx, double q0, double q1, double q2, double q3) {
    const double top = (1.0 - fx) * q0 + fx * q1, bot = (1.0 - fx) * q2 + fx * q3;
    return (1.0 - fy) * top + fy * bot > 0.5;
}

// bit q of the result: mask_sample of q0..q3 = the bits of q
__device__ unsigned mask_table(double fy, double fx) {
    unsigned bits = 0;
    for (int q = 0; q < 16; ++q) bits |= (unsigned)mask_sample(fy, fx, q & 1, (q >> 1) & 1, (q >> 2) & 1, (q >> 3) & 1) << q;
    return bits;
}

// coordinate i of the P of a grid axis of `width` around c: fp64, rounded to fp32
__device__ __forceinline__ float grid_coord(double c, double width, int i, int P) {
    return (float)(c - width / 2.0 + (double)i * width / (double)(P - 1));
}

// the six taps down a column: t[p] = sum_o ky[o] a[p + o] for the RG_RUN pixels of a run out of its RG_RUN + 5 rows
__device__ __forceinline__ void column_taps(const float* ky, const float* a, float* t) {
#pragma unroll
    for (int p = 0; p < RG_RUN; ++p) {
        float s = ky[0] * a[p];
#pragma unroll
        for (int o = 1; o < 6; ++o) s = fmaf(ky[o], a[p + o], s);
        t[p] = s;
    }
}

// Which pixels of a run that begins in frame row y0 are valid at a whole-pixel offset n_y: the row inside the frame with its footprint,
// the same for the column (xin), and the bilinear sample of the pixel's 2 x 2 mask pattern q[p] above 0.5 (`table`: mask_table)
__device__ __forceinline__ unsigned run_valid(bool xin, int y0, int ny, int H, unsigned table, const unsigned* q) {
    unsigned valid = 0;
#pragma unroll
    for (int p = 0; p < RG_RUN; ++p) {
        const int y = y0 + p;
        const bool yin = y < H && y + ny - 2 >= 0 && y + ny + 3 <= H - 1;
        valid |= (unsigned)(xin && yin && ((table >> q[p]) & 1u)) << p;
    }
    return valid;
}

// What a thread adds up at one grid point, in fp64: the count and the five sums over its pixels that are valid in both images.
struct PointSums {
    int n = 0;
    double st = 0.0, sr = 0.0, stt = 0.0, srr = 0.0, srt = 0.0;

    // a run: bit p of `valid` says whether t[p] (the resampled view) and r[p] (the reference) count
    __device__ __forceinline__ void add(unsigned valid, const float* t, const float* r) {
        n += __popc(valid & ((1u << RG_RUN) - 1u));
#pragma unroll
        for (int p = 0; p < RG_RUN; ++p) {
            const bool on = (valid >> p) & 1u;
            float tf = on ? t[p] : 0.f, rf = on ? r[p] : 0.f;
            // The selects stay in fp32: one each, not two on the halves of a double.  A select commutes with the conversion, so the
            // hint changes no value and can go once a compiler keeps the selects in fp32 by itself ("Sums").
            asm("" : "+v"(tf), "+v"(rf));
            const double tm = (double)tf, rm = (double)rf;
            st += tm; sr += rm;
            stt = fma(tm, tm, stt); srr = fma(rm, rm, srr); srt = fma(rm, tm, srt);
        }
    }

    // the wave's six sums {n, sum t, sum r, sum t^2, sum r^2, sum r t} in a fixed order (WaveSums) to red[0..5] (red has 8 entries)
    __device__ __forceinline__ void to_wave(double* red, int lane) const {
        double v[8] = {(double)n, st, sr, stt, srr, srt, 0.0, 0.0};
        WaveSums<8, 0>::run(v, lane);
        if (lane < 8) red[wave_sums_index<8>(lane)] = v[0];
    }
};

// The end of a column j of a level: tot[i P + j][q] = the waves' red[i][w][q] added in order, for the P rows i and the six sums q.  The
// caller's barrier stands between the last to_wave and this, and its next barrier before red is written again.
template <int WAVES>
__device__ __forceinline__ void add_waves(const double (*red)[WAVES][8], double (*tot)[RG_NSUM], int P, int j, int tid) {
    if (tid < P * RG_NSUM) {
        const int i = tid / RG_NSUM, q = tid - i * RG_NSUM;
        double s = 0.0;
        for (int w = 0; w < WAVES; ++w) s += red[i][w][q];
        tot[i * P + j][q] = s;
    }
}

// the score out of the six sums s = {n, sum t, sum r, sum t^2, sum r^2, sum r t} over the common valid pixels, in fp64; -inf without a
// pixel or a variance
__device__ __forceinline__ float mncc_score(const double* s) {
    const double n = s[0];
    float score = -INFINITY;
    if (n > 0.0) {
        const double mt = s[1] / n, mr = s[2] / n;
        const double vt = s[3] / n - mt * mt, vr = s[4] / n - mr * mr;
        if (vt > 0.0 && vr > 0.0) score = (float)((s[5] / n - mr * mt) / (sqrt(vr) * sqrt(vt)));
    }
    return score;
}

// the first maximum in row-major order (strict >) of score[i P + j] at (dys[i], dxs[j]): (cy, cx) becomes its point, and its score is
// returned; without a finite score (cy, cx) stays and -inf is returned
__device__ __forceinline__ float mncc_first_maximum(const float* score, const float* dys, const float* dxs, int P, float& cy, float& cx) {
    float best = -INFINITY;
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j)
            if (score[i * P + j] > best) { best = score[i * P + j]; cy = dys[i]; cx = dxs[j]; }
    return best;
}

// ----------------------------------------------------------------------------- the host side of a level
double level_ratio(int P) {                      // the reference fork's rule: 1 / (P - 2), at least 0.25, and 0.9 where that is not below 1
    const double s = 1.0 / (double)(P - 2);
    return s >= 1.0 ? 0.9 : (s < 0.25 ? 0.25 : s);
}

// the counted arithmetic of one level, per pixel: the pass along rows P 6 2, the pass along columns plus mask plus sums P^2 (6 2 + 20)
double level_flops(int P) { return P * 12.0 + (double)P * P * 32.0; }

}  // namespace
