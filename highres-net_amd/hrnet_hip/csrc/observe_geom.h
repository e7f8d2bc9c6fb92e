// The geometry of the observation model that observe.hip and robust_sr.hip share (include/hrnet_hip.h): the HR
// coordinate of a shift, its split, which samples of a view are valid, and - out of these - whether a sample is COUNTED.  One definition:
// the residual kernel, the adjoint and the robust data term take the same decisions from frame, shift, mask and alpha.
#pragma once
#include "lr_tile.h"

namespace {

constexpr float kMaxCoord = 256.f;                       // RG_DMAX of mncc_common.h: the clamp of split_and_taps

// c = -S d of a shift component: fp64 product, rounded to fp32 (not yet clamped)
__device__ __forceinline__ float hr_coord(int S, float d) { return (float)(-(double)S * (double)d); }

// the split of split_and_taps: the clamp (a NaN goes to a finite value), n = floor, f = c - n exact in fp64
__device__ __forceinline__ void split64(float c, int* n, double* f) {
    const float cc = fminf(fmaxf(c, -kMaxCoord), kMaxCoord);
    const double fl = floor((double)cc);
    *n = (int)fl;
    *f = (double)cc - fl;
}

// a view that counts (view_counts of lr_tile.h) is IN REACH when neither coordinate was clamped
template <int S>
__device__ __forceinline__ bool view_in_reach(const float* shifts, size_t bv) {
    return fabsf(hr_coord(S, shifts[2 * bv])) < kMaxCoord && fabsf(hr_coord(S, shifts[2 * bv + 1])) < kMaxCoord;
}

// sample i of an axis of L LR samples is valid: its S + 5 HR rows S i + n - 2 .. S i + n + S + 2 lie inside 0 .. S L - 1
template <int S>
__device__ __forceinline__ bool sample_valid(int i, int n, int L) {
    const long lo = (long)S * i + n - 2;
    return i >= 0 && i < L && lo >= 0 && lo + S + 4 <= (long)S * L - 1;
}

// The weights and the staged window that observe.hip and observe_shift.hip share.
constexpr int plane_stride(int S) { return S == 2 ? 48 : (S == 3 ? 43 : 40); }

// tap o (-2 .. 3) of split_and_taps before its normalisation, fp64
__device__ __forceinline__ double tap64(int o, double f) {
    const double x = (double)o - f;
    const double px = 3.141592653589793 * x, px3 = 3.141592653589793 * (x / 3.0);
    const double a = x == 0.0 ? 1.0 : sin(px) / px;
    const double b = x == 0.0 ? 1.0 : sin(px3) / px3;
    return fabs(x) >= 3.0 ? 0.0 : a * b;
}

// w_j out of the six raw taps k[0..5] (o = -2 .. 3): normalised as split_and_taps does (the sum in order), box-summed, rounded once
template <int S>
__device__ __forceinline__ float box_weight(const double* k, int j) {
    double sum = 0.0;
#pragma unroll
    for (int o = 0; o < 6; ++o) sum += k[o];
    double w = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int o = j - s;                             // tap index o + 2 = j - s
        if (o >= 0 && o < 6) w += k[o] / sum;
    }
    return (float)(w / (double)S);
}

__device__ __forceinline__ int floor_div(int a, int b) { return (a >= 0 ? a : a - b + 1) / b; }

// What a kernel that only needs `counted` keeps of a view: whether it counts and is in reach (uniform per view), and n of both axes.
struct ViewGeom { bool counts; int ny, nx; };

template <int S>
__device__ __forceinline__ ViewGeom view_geom(const float* alphas, const float* shifts, size_t bv) {
    ViewGeom g;
    g.counts = view_counts(alphas, shifts, bv) && view_in_reach<S>(shifts, bv);
    double f;
    split64(hr_coord(S, shifts[2 * bv]), &g.ny, &f);
    split64(hr_coord(S, shifts[2 * bv + 1]), &g.nx, &f);
    return g;
}

// counted = the view counts, the sample is valid on both axes, and its mask (null: all ones) is non-zero; `at` is the sample's offset
template <int S>
__device__ __forceinline__ bool sample_counted(const ViewGeom& g, const float* masks, size_t at, int iy, int ix, int H, int W) {
    return g.counts && sample_valid<S>(iy, g.ny, H) && sample_valid<S>(ix, g.nx, W) && (!masks || masks[at] != 0.f);
}

}  // namespace
