// Fixed-order sums of several values per lane over a wave, for the reductions whose results must be bit-reproducible (offset_walk.h for
// shift_loss.hip and cl1_loss.hip, registration.hip).
#pragma once
#include <hip/hip_runtime.h>

constexpr int pow2_ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// Wave-wide sums of N (a power of two <= 64) values per lane in N - 1 + log2(64 / N) exchanges instead of 6 N: at step s the lanes
// whose bit s is clear keep the lower half of what is left and hand the upper half over, and the other way round.  Afterwards lane l
// holds the sum over the wave of the value with index sum_s bit_s(l) (N >> (s + 1)).  The order of the additions is fixed.
template <int N, int S>
struct WaveSums {
    static __device__ __forceinline__ void run(double* a, int lane) {
        const bool up = (lane >> S) & 1;
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const double send = up ? a[i] : a[i + N / 2];
            const double keep = up ? a[i + N / 2] : a[i];
            a[i] = keep + __shfl_xor(send, 1 << S);
        }
        WaveSums<N / 2, S + 1>::run(a, lane);
    }
};
template <int S>
struct WaveSums<1, S> {
    static __device__ __forceinline__ void run(double* a, int) {
#pragma unroll
        for (int mask = 1 << S; mask < 64; mask <<= 1) a[0] += __shfl_xor(a[0], mask);
    }
};
template <int N>
__device__ __forceinline__ int wave_sums_index(int lane) {
    int idx = 0;
#pragma unroll
    for (int s = 0, n = N >> 1; n > 0; ++s, n >>= 1) idx += ((lane >> s) & 1) * n;
    return idx;
}
