// The collate kernel and its helpers (collate.hip has the design).  A translation unit defines COLLATE_MASK and includes this file
// once: 0 (collate.hip) gives collate_kernel<VEC, AUG>, 1 (collate_mask.hip) gives collate_mask_kernel<VEC, AUG>, the same text with
// the QM arena and the lr_masks output.  Two kernels from one text in two translation units - not one template with a third parameter
// (that renames the four instances that exist), not one inlined body under two thin kernels (the kernels' `__restrict__` arguments
// become scoped alias information and the instruction schedule moves) and not both in one file (a second kernel with LDS beside
// collate_kernel<true, true> moves that one's schedule too): this way the kernels without masks keep their symbols and, instruction
// for instruction, the code they had (tools/device_code_diff.py).
#ifndef COLLATE_MASK
#error "define COLLATE_MASK (0 or 1) before including collate_kernel.h"
#endif
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
//
// MASK = true is the kernel with LR quality masks (hrn_collate_device_m): min_L more units at the end of the grid, after the SM
// and (with hrs) the HR pieces, one per LR slot.  Unit v of them is the gather of LR unit v with the QM arena (uint8,
// 0 / 1) in place of the LR arena: same plan offset, same window, same code, the uint8 forms of the SM plane, 1 B read and 4 B
// written per element - a block of its own beside the LR blocks, so blocks keep moving comparable bytes.  MASK = false folds all
// of it away: the kernels without masks keep the instructions they had.
template <bool VEC, bool AUG>
#if COLLATE_MASK
__global__ __launch_bounds__(kThreads) void collate_mask_kernel(const uint16_t* __restrict__ lr_arena, long long lr_n,
                                                                const uint16_t* __restrict__ hr_arena, long long hr_n,
                                                                const uint8_t* __restrict__ sm_arena, long long sm_n,
                                                                const uint8_t* __restrict__ qm_arena, const long long* __restrict__ plan,
                                                                const int* __restrict__ codes, int min_L, int S, int scale,
                                                                float* __restrict__ lrs, float* __restrict__ alphas, float* __restrict__ hrs,
                                                                float* __restrict__ maps, float* __restrict__ lr_masks) {
    constexpr bool MASK = true;
#define LR_SIZED (kind == 0 || kind == 3)                // the plane is S a side and a block takes all of it
#define IS_U8 (kind >= 2)                                // the plane comes from a uint8 arena ...
#define ARENA_U8 (kind == 3 ? qm_arena : sm_arena)       // ... this one
#else
__global__ __launch_bounds__(kThreads) void collate_kernel(const uint16_t* __restrict__ lr_arena, long long lr_n,
                                                           const uint16_t* __restrict__ hr_arena, long long hr_n,
                                                           const uint8_t* __restrict__ sm_arena, long long sm_n,
                                                           const long long* __restrict__ plan, const int* __restrict__ codes,
                                                           int min_L, int S, int scale, float* __restrict__ lrs, float* __restrict__ alphas,
                                                           float* __restrict__ hrs, float* __restrict__ maps) {
    constexpr bool MASK = false;
    constexpr float* lr_masks = nullptr;                 // named below only under `MASK &&`
#define LR_SIZED (kind == 0)
#define IS_U8 (kind == 2)
#define ARENA_U8 sm_arena
#endif

    const int b = blockIdx.y, unit = blockIdx.x;
    const long long* p = plan + (size_t)b * (kMeta + min_L);
    const long long side = p[2], r0 = p[3], c0 = p[4];
    const int code = AUG ? codes[b] : 0;                     // uniform per block
    const unsigned SS = (unsigned)S * (unsigned)S;
    const int pieces = scale * scale;                    // S*S pieces per HR / SM plane (S <= 8192: 16 SS fits in 32 bits)
    int kind;                                            // 0 LR, 1 HR, 2 SM, 3 QM (MASK only)
    long long off, n;
    unsigned W, e0;
    float* out;
    if (MASK && unit >= (int)gridDim.x - min_L) {        // the mask plane of LR slot `slot`: the QM arena has the LR arena's offsets and size
        const int slot = unit - ((int)gridDim.x - min_L);
        kind = 3;
        off = p[kMeta + slot];
        n = lr_n;
        W = S;
        e0 = 0;
        out = lr_masks + ((size_t)b * min_L + slot) * SS;
    } else if (unit < min_L) {
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
    const long long mul = LR_SIZED ? 1 : scale, pitch = mul * (bad_row ? 0 : side), sr0 = mul * r0, sc0 = mul * c0;
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
    // A mask unit (kind 3) reads the QM arena at the offsets of an LR unit: hrn_collate_device_m has checked that the QM arena
    // has the LR arena's size lr_n, `off` came from the same plan column and passed the same test against n = lr_n, and the
    // window is the LR window - so the argument for the LR arena is the argument for the QM arena, element for element.
    const bool flip_i = code & 2, flip_j = code & 1;
    if (VEC) {
        if (AUG && (code & 4)) {
            __shared__ __attribute__((aligned(16))) float lds[2 * kTile * kTile];
            const bool lr_unit = LR_SIZED;
            transposed_tiles(kind == 0 ? lr_arena : hr_arena, ARENA_U8, IS_U8, off + sr0 * pitch + sc0, pitch, (int)W, flip_i, flip_j,
                             lr_unit ? 0 : (int)(e0 / SS), lr_unit ? 1 : pieces, out, lds);
            return;
        }
        for (unsigned q = threadIdx.x; q < SS / 4; q += kThreads) {
            const unsigned e = e0 + 4 * q, row = e / W, col = e - row * W;
            const unsigned srow = flip_i ? W - 1 - row : row, scol = flip_j ? W - 4 - col : col;   // col % 4 == 0 and W % 4 == 0
            const long long src = off + (sr0 + srow) * pitch + sc0 + scol;
            *(f32x4*)(out + e) = IS_U8 ? convert4_u8(load4_u8(ARENA_U8, src), flip_j)
                                           : convert4_u16(load4_u16(kind == 0 ? lr_arena : hr_arena, src), flip_j);
        }
    } else {
        for (unsigned i = threadIdx.x; i < SS; i += kThreads) {
            const unsigned e = e0 + i, row = e / W, col = e - row * W;
            const unsigned ip = flip_i ? W - 1 - row : row, jp = flip_j ? W - 1 - col : col;
            const long long src = off + (sr0 + (code & 4 ? jp : ip)) * pitch + sc0 + (code & 4 ? ip : jp);
            out[e] = IS_U8 ? (ARENA_U8[src] ? 1.f : 0.f) : u16_to_f32((kind == 0 ? lr_arena : hr_arena)[src]);
        }
    }
}

#undef LR_SIZED
#undef IS_U8
#undef ARENA_U8

}  // namespace
