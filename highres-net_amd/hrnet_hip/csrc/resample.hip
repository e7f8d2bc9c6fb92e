// Target resampling at cache build (DataLoader.DeviceImagesetCache, resample_targets=True): HR images (uint16) and
// status maps (uint8) stored at n_in x n_in become n_out x n_out in the arenas hrn_collate_device_s reads, so that files stored
// at one HR / LR ratio can feed a model of another target scale.  The filter is separable and comes from the host as a table
// per output sample (first tap, tap count, up to HRN_RESAMPLE_TAPS fp64 weights; hrnet_hip/resample.py), the same for rows and
// columns; this kernel only multiplies and adds.
//
// One block = one 16 x 16 output tile of one image (grid.z = image; offsets from the jobs table, so one launch covers them all).
// The block stages its 32 table rows and the source window they cover in LDS (at most 16 * 2 + 12 = 44 samples a side for the
// steepest pair, 4 -> 2), then every thread sums its own output in a fixed order: deterministic, no atomics.  Runs once per
// cache, so nothing here is tuned beyond that staging.
#include "../../../include/hrnet_hip.h"
#include "common.h"

namespace {

constexpr int kTile = 16;                                // outputs per tile side; kTile * kTile threads
constexpr int kTaps = HRN_RESAMPLE_TAPS;
constexpr int kExt = 48;                                 // staged source window side; a wider one (a foreign table) reads global memory

template <typename T>
__global__ __launch_bounds__(kTile * kTile) void resample_kernel(const T* __restrict__ src, long long src_n, T* __restrict__ dst,
                                                                 long long dst_n, const long long* __restrict__ jobs, int n_in, int n_out,
                                                                 const int* __restrict__ first, const int* __restrict__ count,
                                                                 const double* __restrict__ weights) {
    __shared__ double s_w[2][kTile][kTaps];              // [0] this tile's output rows, [1] its output columns
    __shared__ int s_first[2][kTile], s_count[2][kTile];
    __shared__ uint16_t s_tile[kExt * kExt];
    const long long src_off = jobs[2 * (size_t)blockIdx.z], dst_off = jobs[2 * (size_t)blockIdx.z + 1];
    const long long in2 = (long long)n_in * n_in, out2 = (long long)n_out * n_out;
    if (src_off < 0 || dst_off < 0 || src_off > src_n - in2 || dst_off > dst_n - out2) return;      // the whole block leaves
    const int tid = (int)threadIdx.x, tx = tid % kTile, ty = tid / kTile;
    if (tid < 2 * kTile) {
        const int axis = tid / kTile, i = tid % kTile;
        int j = (int)(axis ? blockIdx.x : blockIdx.y) * kTile + i;
        j = j < n_out ? j : n_out - 1;                   // past the edge: repeat the last row (inside the window, never stored)
        int f = first[j], c = count[j];
        f = f < 0 ? 0 : (f > n_in ? n_in : f);           // whatever the table holds, the taps stay inside the source image
        c = c < 0 ? 0 : (c > kTaps ? kTaps : c);
        c = c > n_in - f ? n_in - f : c;
        s_first[axis][i] = f;
        s_count[axis][i] = c;
        for (int t = 0; t < kTaps; ++t) s_w[axis][i][t] = t < c ? weights[(size_t)j * kTaps + t] : 0.0;
    }
    __syncthreads();
    int lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        lo[a] = n_in;
        hi[a] = 0;
        for (int i = 0; i < kTile; ++i) {
            lo[a] = min(lo[a], s_first[a][i]);
            hi[a] = max(hi[a], s_first[a][i] + s_count[a][i]);
        }
        hi[a] = max(hi[a], lo[a]);
    }
    const int er = hi[0] - lo[0], ec = hi[1] - lo[1];
    const bool staged = er <= kExt && ec <= kExt;         // block-uniform
    const T* img = src + src_off;
    if (staged) {
        for (int i = tid; i < er * ec; i += kTile * kTile) {
            const int r = i / ec, c = i - r * ec;
            s_tile[i] = (uint16_t)img[(size_t)(lo[0] + r) * n_in + lo[1] + c];
        }
        __syncthreads();
    }
    const int jr = (int)blockIdx.y * kTile + ty, jc = (int)blockIdx.x * kTile + tx;
    if (jr >= n_out || jc >= n_out) return;
    const int fr = s_first[0][ty], cr = s_count[0][ty], fc = s_first[1][tx], cc = s_count[1][tx];
    const double* wr = s_w[0][ty];
    const double* wc = s_w[1][tx];
    auto sample = [&](int r, int c) -> unsigned {
        return staged ? (unsigned)s_tile[(r - lo[0]) * ec + (c - lo[1])] : (unsigned)img[(size_t)r * n_in + c];
    };
    T result;
    if (sizeof(T) == 2) {
        double acc = 0.0;
        for (int a = 0; a < cr; ++a) {
            double line = 0.0;
            for (int b = 0; b < cc; ++b) line += wc[b] * (double)sample(fr + a, fc + b);
            acc += wr[a] * line;
        }
        acc = acc > 0.0 ? (acc < 65535.0 ? acc : 65535.0) : 0.0;         // clip (NaN -> 0), then round half to even
        result = (T)(unsigned)rint(acc);
    } else {
        bool clear = cr > 0 && cc > 0;
        for (int a = 0; a < cr; ++a) {
            if (wr[a] == 0.0) continue;
            for (int b = 0; b < cc; ++b) clear = clear && (wc[b] == 0.0 || sample(fr + a, fc + b) != 0);
        }
        result = (T)(clear ? 1 : 0);
    }
    dst[dst_off + (size_t)jr * n_out + jc] = result;
}

bool ratio_ok(int n_in, int n_out) {
    for (int r = 2; r <= 4; ++r)
        for (int s = 2; s <= 4; ++s)
            if ((long long)n_in * s == (long long)n_out * r) return true;
    return false;
}

}  // namespace

extern "C" int hrn_resample_targets(const void* src, int64_t src_elems, void* dst, int64_t dst_elems, int elem_bytes,
                                    const int64_t* jobs, int n_jobs, int n_in, int n_out, const int32_t* first, const int32_t* count,
                                    const double* weights, void* stream) {
    HRN_CHECK(src && dst && jobs && first && count && weights, -2, "hrn_resample_targets: null argument");
    HRN_CHECK(elem_bytes == 1 || elem_bytes == 2, -2, "hrn_resample_targets: elem_bytes must be 1 (uint8 map) or 2 (uint16 image), got %d",
              elem_bytes);
    HRN_CHECK(n_jobs > 0 && n_jobs <= 65535, -2, "hrn_resample_targets: n_jobs must be in 1..65535 (got %d)", n_jobs);
    HRN_CHECK(n_in > 0 && n_in <= 32768 && n_out > 0 && n_out <= 32768, -2,
              "hrn_resample_targets: n_in and n_out must be in 1..32768 (got %d, %d)", n_in, n_out);
    HRN_CHECK(ratio_ok(n_in, n_out), -2, "hrn_resample_targets: n_in : n_out must be R : S with R, S in 2..4 (got %d : %d)", n_in, n_out);
    HRN_CHECK(src_elems >= (int64_t)n_in * n_in && dst_elems >= (int64_t)n_out * n_out, -2,
              "hrn_resample_targets: src / dst hold less than one image");
    HRN_CHECK((uintptr_t)src % elem_bytes == 0 && (uintptr_t)dst % elem_bytes == 0 && (uintptr_t)jobs % 8 == 0 &&
                  (uintptr_t)weights % 8 == 0 && ((uintptr_t)first | (uintptr_t)count) % 4 == 0, -2,
              "hrn_resample_targets: misaligned pointer");
    const unsigned tiles = (unsigned)((n_out + kTile - 1) / kTile);
    const dim3 grid(tiles, tiles, (unsigned)n_jobs);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(resample_kernel<uint16_t>, grid, dim3(kTile * kTile), 0, (hipStream_t)stream, (const uint16_t*)src,
                           (long long)src_elems, (uint16_t*)dst, (long long)dst_elems, (const long long*)jobs, n_in, n_out, first, count,
                           weights);
    else
        hipLaunchKernelGGL(resample_kernel<uint8_t>, grid, dim3(kTile * kTile), 0, (hipStream_t)stream, (const uint8_t*)src,
                           (long long)src_elems, (uint8_t*)dst, (long long)dst_elems, (const long long*)jobs, n_in, n_out, first, count,
                           weights);
    HRN_LAUNCH_CHECK();
    return 0;
}
