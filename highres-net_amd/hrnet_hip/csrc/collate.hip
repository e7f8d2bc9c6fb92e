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
//
// Augmentation (hrn_collate_device_a; hrnet_hip/augment.py gives the rule): one code t in 0..7 per sample, the same for every
// plane of the sample, acting on the cropped window of side n (S for LR, k*S for HR / SM):
//     i' = t & 2 ? n-1-i : i,   j' = t & 1 ? n-1-j : j,   out[i][j] = in[t & 4 ? (j', i') : (i', j')].
// The code is uniform per block (blockIdx.y is the sample), so the kernel branches once per block:
//   t in 0..3  stays on the vector path above.  A row flip is an address; a column flip mirrors the column (col -> n-4-col,
//              a start of arbitrary alignment, which load4_* take anyway) and reverses the four samples of the lane.
//   t in 4..7  (vector path) goes through LDS in kTile x kTile sub-tiles, so that global reads stay contiguous 8-byte (LR / HR)
//              or 4-byte (SM) loads along source rows and global writes stay whole 16-byte stores along output rows.  The plane
//              of side n is cut into ceil(n / kTile)^2 tiles (edge tiles are multiples of 4 a side since n % 4 == 0); an LR block
//              takes all tiles of its plane, HR / SM block p of k*k takes tiles p, p + k*k, ... (4 each whenever S % 32 == 0),
//              so the grid and "one launch, no atomics" do not change.  Per tile: a lane loads 4 samples of one source row,
//              converts them and writes them down one column of the f32 tile with 4 ds_write_b32; after one barrier it reads a
//              row of the tile with one ds_read_b128 and stores it.  Two tile buffers alternate, so one barrier per tile
//              suffices (a wave can only reach the write of tile t+2 after every wave has finished reading tile t).
//     LDS layout (swizzle_tile.h): pitch kTile = 32 dwords (no padding - ds_read_b128 needs 16-byte rows), the 16-byte slot of element (R, C)
//              XOR-swizzled with the row block: dword R*32 + 4*((C/4) ^ (R/4)) + C%4.  Derived conflict count: 0 and 0.
//              - ds_write_b32, bank (a/4) % 32, groups = 32-lane halves: a half holds 4 tile columns c..c+3 (c % 4 == 0) times
//                8 row blocks R/4 = 0..7; the bank is 4*((c/4) ^ (R/4)) + c%4 - the XOR with a constant permutes 0..7, so the 32
//                lanes hit 32 distinct banks.  (Unswizzled they would hit 4: an 8-way conflict.)  The compiler pairs the four
//                column writes of a lane into two ds_write2_b32; each access of a pair is banked like a ds_write_b32.
//              - ds_read_b128, bank (a/4) % 64, four 16-lane groups {0-3,12-15,20-27}, ...: a group reads quarter-rows
//                (R0, slots 0-3), (R0+1, 4-7), (R0+2, 4-7), (R0+3, 0-3) of four rows that share R/4; rows alternate between the
//                two 128-byte halves of the 256-byte bank row, and the XOR with the common R/4 maps {0-3} u {4-7} onto 0..7 in
//                each half: 16 lanes, 16 distinct slots.
//   The non-vector path applies the index map per element.  A code outside 0..7 makes every plane of that sample NaN (the
//   host cannot look at a device array without a synchronise), as a bad plan row does; other samples are not affected.
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): with codes, collate_kernel<true, true> 34 VGPRs, 8 KiB LDS (two tiles),
// <false, true> 22 VGPRs, no LDS; without codes <true, false> / <false, false> 30 / 22 VGPRs, no LDS, as before augmentation.
// No instance uses scratch.
#include "../../../include/hrnet_hip.h"
#include "common.h"
#include "swizzle_tile.h"                                // kTile, tile_at (shared with dihedral.hip)

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

__device__ __forceinline__ f32x4 convert4_u16(uint64_t u, bool reversed) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = u16_to_f32((unsigned)(u >> (16 * j)) & 0xffffu);
    if (reversed) v = f32x4{v[3], v[2], v[1], v[0]};
    return v;
}
__device__ __forceinline__ f32x4 convert4_u8(uint32_t m, bool reversed) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (m >> (8 * j)) & 0xffu ? 1.f : 0.f;
    if (reversed) v = f32x4{v[3], v[2], v[1], v[0]};
    return v;
}

// Codes 4..7 on the vector path: tiles t0, t0 + tstep, ... of the n x n output plane `out`, out[i][j] = window[j'][i'] with
// `window` the element index of the window's corner in the arena (n % 4 == 0).  A lane reads window[sr][sc .. sc+3] with
// 0 <= sr < n and 0 <= sc <= n - 4: four samples of one row of the window, which the caller has checked to lie inside the
// stored image and that image inside the arena - so element window + sr*pitch + sc + 3 is in the arena, which is all load4_* need.
__device__ __forceinline__ void transposed_tiles(const uint16_t* __restrict__ a16, const uint8_t* __restrict__ a8, bool is_map,
                                                 long long window, long long pitch, int n, bool flip_i, bool flip_j, int t0, int tstep,
                                                 float* __restrict__ out, float* lds) {
    const int nts = (n + kTile - 1) / kTile, ntiles = nts * nts;
    const int lr = threadIdx.x >> 3, lq = (threadIdx.x & 7) << 2;        // a lane's row and first column of 4, on both sides
    int buf = 0;
    for (int t = t0; t < ntiles; t += tstep, buf ^= 1) {
        float* tile = lds + buf * (kTile * kTile);
        const int oi0 = (t / nts) * kTile, oj0 = (t % nts) * kTile;       // output corner of the tile
        const int h = min(kTile, n - oi0), w = min(kTile, n - oj0);
        if (lr < w && lq < h) {                                          // source row <-> output column j, 4 source columns <-> rows i..i+3
            const int j = oj0 + lr, i = oi0 + lq;
            const int sr = flip_j ? n - 1 - j : j, sc = flip_i ? n - 4 - i : i;
            const long long src = window + (long long)sr * pitch + sc;
            const f32x4 v = is_map ? convert4_u8(load4_u8(a8, src), flip_i) : convert4_u16(load4_u16(a16, src), flip_i);
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[tile_at(lq + k, lr)] = v[k];
        }
        __syncthreads();
        if (lr < h && lq < w) *(f32x4*)(out + (size_t)(oi0 + lr) * n + oj0 + lq) = *(const f32x4*)(tile + tile_at(lr, lq));
    }
}

// AUG = false is the kernel without codes (hrn_collate_device_s): `code` is the constant 0 and everything that serves the codes
// folds away, LDS included, so identity batches run the instructions they ran before augmentation existed.
template <bool VEC, bool AUG>
__global__ __launch_bounds__(kThreads) void collate_kernel(const uint16_t* __restrict__ lr_arena, long long lr_n,
                                                           const uint16_t* __restrict__ hr_arena, long long hr_n,
                                                           const uint8_t* __restrict__ sm_arena, long long sm_n,
                                                           const long long* __restrict__ plan, const int* __restrict__ codes,
                                                           int min_L, int S, int scale, float* __restrict__ lrs, float* __restrict__ alphas,
                                                           float* __restrict__ hrs, float* __restrict__ maps) {
    const int b = blockIdx.y, unit = blockIdx.x;
    const long long* p = plan + (size_t)b * (kMeta + min_L);
    const long long side = p[2], r0 = p[3], c0 = p[4];
    const int code = AUG ? codes[b] : 0;                     // uniform per block
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
    const bool bad = (unsigned)code > 7u || (off >= 0 && (bad_row || (off & 3) || off > n - pitch * pitch));
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
    // From here on the window [sr0, sr0 + W) x [sc0, sc0 + W) lies inside the stored pitch x pitch image (bad_row) and that image
    // inside the arena (off <= n - pitch^2).  Every code reads source positions (i', j') or (j', i') with both in 0..W-1, i.e.
    // inside the window; the vector forms read 4 consecutive samples of one window row starting at a column <= W - 4.
    const bool flip_i = code & 2, flip_j = code & 1;
    if (VEC) {
        if (AUG && (code & 4)) {
            __shared__ __attribute__((aligned(16))) float lds[2 * kTile * kTile];
            const bool lr_unit = kind == 0;
            transposed_tiles(kind == 0 ? lr_arena : hr_arena, sm_arena, kind == 2, off + sr0 * pitch + sc0, pitch, (int)W, flip_i, flip_j,
                             lr_unit ? 0 : (int)(e0 / SS), lr_unit ? 1 : pieces, out, lds);
            return;
        }
        for (unsigned q = threadIdx.x; q < SS / 4; q += kThreads) {
            const unsigned e = e0 + 4 * q, row = e / W, col = e - row * W;
            const unsigned srow = flip_i ? W - 1 - row : row, scol = flip_j ? W - 4 - col : col;   // col % 4 == 0 and W % 4 == 0
            const long long src = off + (sr0 + srow) * pitch + sc0 + scol;
            *(f32x4*)(out + e) = kind == 2 ? convert4_u8(load4_u8(sm_arena, src), flip_j)
                                           : convert4_u16(load4_u16(kind == 0 ? lr_arena : hr_arena, src), flip_j);
        }
    } else {
        for (unsigned i = threadIdx.x; i < SS; i += kThreads) {
            const unsigned e = e0 + i, row = e / W, col = e - row * W;
            const unsigned ip = flip_i ? W - 1 - row : row, jp = flip_j ? W - 1 - col : col;
            const long long src = off + (sr0 + (code & 4 ? jp : ip)) * pitch + sc0 + (code & 4 ? ip : jp);
            out[e] = kind == 2 ? (sm_arena[src] ? 1.f : 0.f) : u16_to_f32((kind == 0 ? lr_arena : hr_arena)[src]);
        }
    }
}

}  // namespace

extern "C" int hrn_collate_device_a(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                                    const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale,
                                    float* lrs, float* alphas, float* hrs, float* maps, const int32_t* codes, void* stream) {
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
    HRN_CHECK((uintptr_t)codes % 4 == 0, -2, "hrn_collate_device: codes must be 4-byte aligned");
    const bool vec = S % 4 == 0 && ((uintptr_t)lrs | (uintptr_t)hrs | (uintptr_t)maps) % 16 == 0;
    const int pieces = scale * scale;
    const dim3 grid((unsigned)(min_L + pieces + (hrs ? pieces : 0)), (unsigned)B);
    auto kernel = vec ? (codes ? collate_kernel<true, true> : collate_kernel<true, false>)
                      : (codes ? collate_kernel<false, true> : collate_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, lr_arena, (long long)lr_elems, hr_arena, (long long)hr_elems,
                       sm_arena, (long long)sm_elems, (const long long*)plan, (const int*)codes, min_L, S, scale, lrs, alphas, hrs, maps);
    HRN_LAUNCH_CHECK();
    return 0;
}
