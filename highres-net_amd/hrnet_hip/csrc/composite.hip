// Cloud-free composite reference frame: the per-pixel lower median over the CLEAR pixels of the first n_ref views, and the views with
// their masked pixels filled from it (hrn_masked_composite, include/hrnet_hip.h).  (No counterpart in the reference, whose HRNet.py:200
// takes the plain median of lrs[:, :9]; with no masks, no alphas and n_ref = 9 this kernel gives that median bit for bit.)
//
// One launch, one thread per pixel, a block inside one sample (so the sample's alphas are wave-uniform).  A thread loads its n = min(V,
// n_ref) values and masks once and keeps them: the values for `filled`, the masks as one bit each.  The key of a view that does not vote
// is +inf, so after sorting the c voters are the first c keys and the lower median is key (c - 1) / 2.  Who votes is decided BEFORE the
// sort - the candidates; if there is none, the real views; if there is none either, all n - so there is one sort per pixel.  The sort is a
// fully unrolled network on registers: the 25-exchange network of median_kernel (stem.hip) for n <= 9, Batcher's odd-even merge sort
// for 16 and 32 keys (the 32-key sort is two 16-key sorts and Batcher's merge); only keys 0..(NK - 1) / 2 are read afterwards, so the
// compiler drops the exchanges that feed nothing else.  No array is indexed by a run-time value.
// Memory-bound: 4 B * HW * (n + n + 2) per sample for ref and count, 4 B * HW * (2 V + V + 2) with `filled`.
#include "../../../include/hrnet_hip.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ void cswap(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

template <int NK> __device__ __forceinline__ void sort_keys(float (&v)[NK]) {
    if constexpr (NK == 9) {
        // the network of median_kernel (stem.hip), verified by the 0-1 principle in tests/test_host_logic.py
        cswap(v[0], v[3]); cswap(v[1], v[7]); cswap(v[2], v[5]); cswap(v[4], v[8]);
        cswap(v[0], v[7]); cswap(v[2], v[4]); cswap(v[3], v[8]); cswap(v[5], v[6]);
        cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[4], v[5]); cswap(v[7], v[8]);
        cswap(v[1], v[4]); cswap(v[3], v[6]); cswap(v[5], v[7]);
        cswap(v[0], v[1]); cswap(v[2], v[4]); cswap(v[3], v[5]); cswap(v[6], v[8]);
        cswap(v[2], v[3]); cswap(v[4], v[5]); cswap(v[6], v[7]);
        cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
    } else {
        // Batcher's odd-even merge sort for a power of two (restated and checked by the 0-1 principle in tests/test_composite_host.py);
        // every bound is a compile-time constant, so the loops unroll into 63 (NK = 16) / 191 (NK = 32) exchanges of named registers
        static_assert(NK == 16 || NK == 32, "networks for 9, 16 and 32 keys");
#pragma unroll
        for (int p = 1; p < NK; p *= 2)
#pragma unroll
            for (int k = p; k >= 1; k /= 2)
#pragma unroll
                for (int j = k % p; j + k < NK; j += 2 * k)
#pragma unroll
                    for (int i = 0; i < k; ++i)
                        if (i + j + k < NK && (i + j) / (2 * p) == (i + j + k) / (2 * p)) cswap(v[i + j], v[i + j + k]);
    }
}

// views, masks, filled [B][V][hw]; alphas [B][V]; ref, count [B][hw]; blockIdx.x = b * tiles + tile of 256 pixels
template <int NK>
__global__ __launch_bounds__(256) void masked_composite_kernel(const float* __restrict__ views, const float* __restrict__ masks,
                                                               const float* __restrict__ alphas, int V, int n, size_t hw, unsigned tiles,
                                                               float* __restrict__ ref, float* __restrict__ count,
                                                               float* __restrict__ filled) {
    const unsigned b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const size_t pix = (size_t)t * 256 + threadIdx.x;
    if (pix >= hw) return;
    const float* src = views + (size_t)b * V * hw + pix;
    const float* msk = masks ? masks + (size_t)b * V * hw + pix : nullptr;
    const float* al = alphas ? alphas + (size_t)b * V : nullptr;
    const unsigned all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    unsigned real = all;                        // bit v: view v < n is real (uniform over the block)
    if (al) {
        real = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i)
            if (i < n && al[i] != 0.f) real |= 1u << i;
    }
    float val[NK];
    unsigned clear = all;                       // bit v: the pixel of view v < n is clear
#pragma unroll
    for (int i = 0; i < NK; ++i) val[i] = i < n ? src[(size_t)i * hw] : 0.f;
    if (msk) {
        clear = 0;
#pragma unroll
        for (int i = 0; i < NK; ++i)
            if (i < n && msk[(size_t)i * hw] != 0.f) clear |= 1u << i;
    }
    const unsigned cand = real & clear;
    const unsigned vote = cand ? cand : (real ? real : all);
    float key[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) key[i] = (vote >> i) & 1u ? val[i] : __builtin_inff();
    sort_keys<NK>(key);
    const int k = (__popc(vote) - 1) >> 1;      // lower median of the voters
    float out = key[0];
#pragma unroll
    for (int i = 1; i <= (NK - 1) / 2; ++i) out = (i == k) ? key[i] : out;
    ref[(size_t)b * hw + pix] = out;
    if (count) count[(size_t)b * hw + pix] = (float)__popc(cand);
    if (filled) {
        float* dst = filled + (size_t)b * V * hw + pix;
        const unsigned hole = real & ~clear;    // real views whose pixel is masked
#pragma unroll
        for (int i = 0; i < NK; ++i)
            if (i < n) dst[(size_t)i * hw] = (hole >> i) & 1u ? out : val[i];
        // the views that do not vote: read once, filled where a real view is masked
        for (int v = n; v < V; ++v) {
            const float x = src[(size_t)v * hw];
            const bool fill = msk && msk[(size_t)v * hw] == 0.f && (!al || al[v] != 0.f);
            dst[(size_t)v * hw] = fill ? out : x;
        }
    }
}

}  // namespace

int hrn_launch_masked_composite(const float* views, const float* masks, const float* alphas, int B, int V, int H, int W, int n_ref, float* ref,
                                float* count, float* filled, hipStream_t stream) {
    const size_t hw = (size_t)H * W, tiles = (hw + 255) / 256;
    HRN_CHECK(tiles * (size_t)B < ((size_t)1 << 31), -2, "hrn_masked_composite: %d samples of %d x %d exceed one launch", B, H, W);
    const int n = V < n_ref ? V : n_ref;
    const double px = (double)B * (double)hw;
    HrnProfScope prof("masked_composite", 0.0, px * 4 * (filled ? (masks ? 3.0 : 2.0) * V + 2 : (masks ? 2.0 : 1.0) * n + 2), stream);
    const dim3 grid((unsigned)(tiles * B)), block(256);
    if (n <= 9)
        hipLaunchKernelGGL(masked_composite_kernel<9>, grid, block, 0, stream, views, masks, alphas, V, n, hw, (unsigned)tiles, ref, count, filled);
    else if (n <= 16)
        hipLaunchKernelGGL(masked_composite_kernel<16>, grid, block, 0, stream, views, masks, alphas, V, n, hw, (unsigned)tiles, ref, count, filled);
    else
        hipLaunchKernelGGL(masked_composite_kernel<32>, grid, block, 0, stream, views, masks, alphas, V, n, hw, (unsigned)tiles, ref, count, filled);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_masked_composite(const float* views, const float* masks, const float* alphas, int B, int V, int H, int W, int n_ref, float* ref,
                                    float* count, float* filled, void* stream) {
    HRN_CHECK(B > 0 && V > 0 && H > 0 && W > 0, -2, "hrn_masked_composite: empty input B=%d V=%d H=%d W=%d", B, V, H, W);
    HRN_CHECK(n_ref >= 1 && n_ref <= 32, -2, "hrn_masked_composite: n_ref %d outside 1..32", n_ref);
    HRN_CHECK(views && ref, -2, "hrn_masked_composite: null argument");
    return hrn_launch_masked_composite(views, masks, alphas, B, V, H, W, n_ref, ref, count, filled, (hipStream_t)stream);
}
