// Batch assembly from the HBM-resident imageset cache (DataLoader.DeviceImagesetCache): the device side of
// ImagesetDataset.load_batch.  The PNGs were decoded once into three arenas (LR and HR uint16, SM uint8); a small plan table
// (one row per sample, built on the host from the same numpy RNG draws as the host path) says which stored views fill the
// min_L slots and where the patch sits.  ONE launch writes lrs (B,min_L,S,S), alphas (B,min_L), hrs and maps (B,kS,kS), f32,
// padding included, with the host's value rules: (float)((double)u / 65535.0) for LR / HR, (u != 0) for the map.  k is the
// target scale (2, 3 or 4; hrn_collate_device is k = 3): HR / SM are stored at k * side.
//
// Work unit = one block per (sample, S*S output elements): the min_L LR slots, then the k*k S*S pieces of the SM plane, then
// (with hrs) the k*k pieces of the HR plane, so every block moves the same bytes.  A gather + convert: 2 B (LR / HR) or 1 B (SM)
// read and 4 B written per element, no reuse - bound by HBM and, at these sizes, by the launch itself.  Vector path (S % 4 == 0):
// a lane owns 4 consecutive outputs of one row, reads them with one or two aligned 8-byte (uint16) / 4-byte (uint8) loads
// (the patch corner is arbitrary, so the 4 samples are funnel-shifted out of two words) and writes one 16-byte store.
#include "../../../include/hrnet_hip.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMeta = HRN_COLLATE_META;                 // plan row: hr_off, sm_off, side, row, col, then min_L LR offsets
constexpr long long kMaxSide = 1 << 20;                  // a larger stored side is a bad row (keeps 16 side^2 far from int64 overflow)

// 4 consecutive samples from element i of an arena whose images start at multiples of 4 elements and whose size is a multiple
// of 4: the second word is read only when i is not 4-aligned, and then it holds element i + 3, so it lies inside the arena.
__device__ __forceinline__ uint64_t load4_u16(const uint16_t* __restrict__ a, long long i) {
    const uint64_t* w = (const uint64_t*)a + (i >> 2);
    const int sh = (int)(i & 3);
    uint64_t v = w[0];
    if (sh) v = (v >> (16 * sh)) | (w[1] << (16 * (4 - sh)));
    return v;
}
__device__ __forceinline__ uint32_t load4_u8(const uint8_t* __restrict__ a, long long i) {
    const uint32_t* w = (const uint32_t*)a + (i >> 2);
    const int sh = (int)(i & 3);
    uint32_t v = w[0];
    if (sh) v = (v >> (8 * sh)) | (w[1] << (8 * (4 - sh)));
    return v;
}
// skimage.img_as_float(uint16).astype(float32), exactly as the host path rounds it (f64 divide, then f32)
__device__ __forceinline__ float u16_to_f32(unsigned u) { return (float)((double)u / 65535.0); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void collate_kernel(const uint16_t* __restrict__ lr_arena, long long lr_n,
                                                           const uint16_t* __restrict__ hr_arena, long long hr_n,
                                                           const uint8_t* __restrict__ sm_arena, long long sm_n,
                                                           const long long* __restrict__ plan, int min_L, int S, int scale,
                                                           float* __restrict__ lrs, float* __restrict__ alphas,
                                                           float* __restrict__ hrs, float* __restrict__ maps) {
    const int b = blockIdx.y, unit = blockIdx.x;
    const long long* p = plan + (size_t)b * (kMeta + min_L);
    const long long side = p[2], r0 = p[3], c0 = p[4];
    const unsigned SS = (unsigned)S * (unsigned)S;
    const int pieces = scale * scale;                    // S*S pieces per HR / SM plane (S <= 8192: 16 SS fits in 32 bits)
    int kind;                                            // 0 LR, 1 HR, 2 SM
    long long off, n;
    unsigned W, e0;
    float* out;
    if (unit < min_L) {
        kind = 0;
        off = p[kMeta + unit];
        n = lr_n;
        W = S;
        e0 = 0;
        out = lrs + ((size_t)b * min_L + unit) * SS;
        if (threadIdx.x == 0) alphas[(size_t)b * min_L + unit] = off >= 0 ? 1.f : 0.f;
    } else {
        const int k = unit - min_L;
        kind = k < pieces ? 2 : 1;
        off = kind == 1 ? p[0] : p[1];
        n = kind == 1 ? hr_n : sm_n;
        W = (unsigned)scale * S;
        e0 = (unsigned)(k % pieces) * SS;
        out = (kind == 1 ? hrs : maps) + (size_t)b * pieces * SS;
    }
    // a plan row that points outside its arena or a corner outside the stored image: NaN, never an out-of-bounds read.  Every
    // comparison is arranged so that no int64 sum overflows, whatever the row holds (side is bounded first: pitch <= 2^22).
    const bool bad_row = side <= 0 || side > kMaxSide || r0 < 0 || c0 < 0 || r0 > side - S || c0 > side - S;
    const long long mul = kind == 0 ? 1 : scale, pitch = mul * (bad_row ? 0 : side), sr0 = mul * r0, sc0 = mul * c0;
    const bool bad = off >= 0 && (bad_row || (off & 3) || off > n - pitch * pitch);
    if (off < 0 || bad) {                                // padding slot (alpha 0) / sample without HR: zeros
        const float fill = bad ? __builtin_nanf("") : 0.f;
        if (VEC) {
            const f32x4 z = {fill, fill, fill, fill};
            for (unsigned q = threadIdx.x; q < SS / 4; q += kThreads) *(f32x4*)(out + e0 + 4 * q) = z;
        } else {
            for (unsigned e = threadIdx.x; e < SS; e += kThreads) out[e0 + e] = fill;
        }
        return;
    }
    if (VEC) {
        for (unsigned q = threadIdx.x; q < SS / 4; q += kThreads) {
            const unsigned e = e0 + 4 * q, row = e / W, col = e - row * W;
            const long long src = off + (sr0 + row) * pitch + sc0 + col;
            f32x4 v;
            if (kind == 2) {
                const uint32_t m = load4_u8(sm_arena, src);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (m >> (8 * j)) & 0xffu ? 1.f : 0.f;
            } else {
                const uint64_t u = load4_u16(kind == 0 ? lr_arena : hr_arena, src);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = u16_to_f32((unsigned)(u >> (16 * j)) & 0xffffu);
            }
            *(f32x4*)(out + e) = v;
        }
    } else {
        for (unsigned i = threadIdx.x; i < SS; i += kThreads) {
            const unsigned e = e0 + i, row = e / W, col = e - row * W;
            const long long src = off + (sr0 + row) * pitch + sc0 + col;
            out[e] = kind == 2 ? (sm_arena[src] ? 1.f : 0.f) : u16_to_f32((kind == 0 ? lr_arena : hr_arena)[src]);
        }
    }
}

}  // namespace

extern "C" int hrn_collate_device_s(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                                    const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale,
                                    float* lrs, float* alphas, float* hrs, float* maps, void* stream) {
    HRN_CHECK(hrn_scale_ok(scale), -2, "hrn_collate_device: scale must be 2, 3 or 4 (got %d)", scale);
    HRN_CHECK(lr_arena && sm_arena && plan && lrs && alphas && maps, -2, "hrn_collate_device: null argument");
    HRN_CHECK(!hrs || hr_arena, -2, "hrn_collate_device: hrs given without an HR arena");
    HRN_CHECK(B > 0 && B <= 65535, -2, "hrn_collate_device: B must be in 1..65535 (got %d)", B);
    HRN_CHECK(min_L > 0 && min_L <= (1 << 20), -2, "hrn_collate_device: min_L must be in 1..2^20 (got %d)", min_L);
    HRN_CHECK(S > 0 && S <= 8192, -2, "hrn_collate_device: S must be in 1..8192 (got %d)", S);
    HRN_CHECK(lr_elems > 0 && sm_elems > 0 && hr_elems >= 0 && lr_elems % 4 == 0 && hr_elems % 4 == 0 && sm_elems % 4 == 0, -2,
              "hrn_collate_device: arena sizes must be positive multiples of 4 elements");
    HRN_CHECK(((uintptr_t)lr_arena | (uintptr_t)hr_arena) % 8 == 0 && (uintptr_t)sm_arena % 4 == 0, -2,
              "hrn_collate_device: arenas must be 8-byte (uint16) / 4-byte (uint8) aligned");
    const bool vec = S % 4 == 0 && ((uintptr_t)lrs | (uintptr_t)hrs | (uintptr_t)maps) % 16 == 0;
    const int pieces = scale * scale;
    const dim3 grid((unsigned)(min_L + pieces + (hrs ? pieces : 0)), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(collate_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, lr_arena, (long long)lr_elems, hr_arena,
                           (long long)hr_elems, sm_arena, (long long)sm_elems, (const long long*)plan, min_L, S, scale, lrs, alphas, hrs,
                           maps);
    else
        hipLaunchKernelGGL(collate_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, lr_arena, (long long)lr_elems, hr_arena,
                           (long long)hr_elems, sm_arena, (long long)sm_elems, (const long long*)plan, min_L, S, scale, lrs, alphas, hrs,
                           maps);
    HRN_LAUNCH_CHECK();
    return 0;
}
