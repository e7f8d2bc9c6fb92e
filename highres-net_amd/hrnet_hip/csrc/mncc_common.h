// What the two masked-NCC registration paths share (DESIGN.md sections 7f and 7g): registration.hip, a view resident in one CU's LDS, and
// registration_scene.hip, frames of any size in tiles.  The split of a coordinate into whole pixels, fraction and six taps, the table
// of the bilinear mask test, a grid coordinate, the score out of the six sums and the first-maximum rule are written once, so that the
// two paths cannot drift apart.  Everything is in an unnamed namespace: each translation unit gets its own copy, as before.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)      // every fused multiply-add of both paths is written out: kernels that share a level must round alike

namespace {

constexpr int RG_NSUM = 6;                      // n, sum t, sum r, sum t^2, sum r^2, sum r t
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

// bit q of the result: (1 - fy) ((1 - fx) q0 + fx q1) + fy ((1 - fx) q2 + fx q3) > 0.5, q0..q3 the bits of q: the mask at (y, x), (y, x + 1),
// (y + 1, x), (y + 1, x + 1).  fp64, in the order the definition writes it.
__device__ unsigned mask_table(double fy, double fx) {
    unsigned bits = 0;
    for (int q = 0; q < 16; ++q) {
        const double q0 = q & 1, q1 = (q >> 1) & 1, q2 = (q >> 2) & 1, q3 = (q >> 3) & 1;
        const double top = (1.0 - fx) * q0 + fx * q1, bot = (1.0 - fx) * q2 + fx * q3;
        const double v = (1.0 - fy) * top + fy * bot;
        bits |= (unsigned)(v > 0.5) << q;
    }
    return bits;
}

// coordinate i of the P of a grid axis of `width` around c: fp64, rounded to fp32
__device__ __forceinline__ float grid_coord(double c, double width, int i, int P) {
    return (float)(c - width / 2.0 + (double)i * width / (double)(P - 1));
}

}  // namespace

// The next two are macros, not functions: as inlined functions they leave registration.hip's search kernel with the same instructions in
// another register allocation, and tools/device_code_diff.py holds that kernel to its code of before the split.
//
// score = the score out of the six sums s = {n, sum t, sum r, sum t^2, sum r^2, sum r t} over the common valid pixels, in fp64; -inf
// without a pixel or a variance
#define MNCC_SCORE(s, score)                                                                                        \
    do {                                                                                                            \
        const double n = (s)[0];                                                                                    \
        (score) = -INFINITY;                                                                                        \
        if (n > 0.0) {                                                                                              \
            const double mt = (s)[1] / n, mr = (s)[2] / n;                                                          \
            const double vt = (s)[3] / n - mt * mt, vr = (s)[4] / n - mr * mr;                                      \
            if (vt > 0.0 && vr > 0.0) (score) = (float)(((s)[5] / n - mr * mt) / (sqrt(vr) * sqrt(vt)));            \
        }                                                                                                           \
    } while (0)

// the first maximum in row-major order (strict >) of score[i P + j] at (dys[i], dxs[j]): (cy, cx) becomes its point and best its
// score; without a finite score (cy, cx) stays and best is -inf
#define MNCC_FIRST_MAXIMUM(score, dys, dxs, P, best, cy, cx)                                                        \
    do {                                                                                                            \
        (best) = -INFINITY;                                                                                         \
        for (int i = 0; i < (P); ++i)                                                                               \
            for (int j = 0; j < (P); ++j)                                                                           \
                if ((score)[i * (P) + j] > (best)) { (best) = (score)[i * (P) + j]; (cy) = (dys)[i]; (cx) = (dxs)[j]; } \
    } while (0)
