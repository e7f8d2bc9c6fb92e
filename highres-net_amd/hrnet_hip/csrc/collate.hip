// Batch assembly from the HBM-resident imageset cache (DataLoader.DeviceImagesetCache): the device side of
// ImagesetDataset.load_batch.  The PNGs were decoded once into three arenas (LR and HR uint16, SM uint8; a fourth, QM uint8, with the
// LR quality masks on); a small plan table (one row per sample, built on the host from the same numpy RNG draws as the host path)
// says which stored views fill the min_L slots and where the patch sits.  ONE launch writes lrs (B,min_L,S,S), alphas (B,min_L),
// hrs and maps (B,kS,kS), f32, padding included, with the host's value rules: (float)((double)u / 65535.0) for LR / HR, (u != 0)
// for the map.  k is the target scale (2, 3 or 4; hrn_collate_device is k = 3): HR / SM are stored at k * side.
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
//
// LR quality masks (hrn_collate_device_m): a fourth arena QM - uint8, one byte per LR sample, 0 / 1, at exactly the LR arena's element
// offsets, so the plan row needs no new column - and a fifth output lr_masks (B,min_L,S,S).  The grid grows by min_L units at its end
// (after the SM and, with hrs, the HR pieces): mask unit v of a sample is the gather of side n = S of LR unit v - same plan offset,
// same window, same code - from the QM arena through the uint8 forms of the SM plane (load4_u8 / convert4_u8, and for codes 4..7
// transposed_tiles with is_map true and the QM arena as a8).  A unit of its own beside the LR unit, not a second loop inside it: a
// mask block reads 1 B and writes 4 B per element where an LR block reads 2 B and writes 4 B, so blocks keep moving comparable
// bytes; still one launch, no atomics, no second pass.  The bank argument above does not depend on where a tile's samples come
// from: a mask plane uses the tiles of an LR plane (ceil(S / kTile)^2 of them, f32, written down columns and read along rows by the
// same lanes), so the derived conflict count stays 0 and 0.  Bounds: the entry point requires qm_elems == lr_elems, so the test
// `off > n - pitch^2` against n = lr_elems that admits an LR unit admits the mask unit with the same offsets.  The kernel text is
// collate_kernel.h, compiled here without masks and in collate_mask.hip with them (that file says why two translation units).
#include "../../../include/hrnet_hip.h"
#include "collate_mask.h"
#define COLLATE_MASK 0
#include "collate_kernel.h"                              // collate_kernel<VEC, AUG>; collate_mask.hip holds the instances with masks

extern "C" int hrn_collate_device_m(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                                    const uint8_t* sm_arena, int64_t sm_elems, const uint8_t* qm_arena, int64_t qm_elems, const int64_t* plan,
                                    int B, int min_L, int S, int scale, float* lrs, float* alphas, float* hrs, float* maps, float* lr_masks,
                                    const int32_t* codes, void* stream) {
    HRN_CHECK(hrn_scale_ok(scale), -2, "hrn_collate_device: scale must be 2, 3 or 4 (got %d)", scale);
    HRN_CHECK(lr_arena && sm_arena && plan && lrs && alphas && maps, -2, "hrn_collate_device: null argument");
    HRN_CHECK(!hrs || hr_arena, -2, "hrn_collate_device: hrs given without an HR arena");
    HRN_CHECK(!qm_arena == !lr_masks, -2, "hrn_collate_device: lr_masks and the QM arena go together (one of them is null)");
    HRN_CHECK(B > 0 && B <= 65535, -2, "hrn_collate_device: B must be in 1..65535 (got %d)", B);
    HRN_CHECK(min_L > 0 && min_L <= (1 << 20), -2, "hrn_collate_device: min_L must be in 1..2^20 (got %d)", min_L);
    HRN_CHECK(S > 0 && S <= 8192, -2, "hrn_collate_device: S must be in 1..8192 (got %d)", S);
    HRN_CHECK(lr_elems > 0 && sm_elems > 0 && hr_elems >= 0 && lr_elems % 4 == 0 && hr_elems % 4 == 0 && sm_elems % 4 == 0, -2,
              "hrn_collate_device: arena sizes must be positive multiples of 4 elements");
    HRN_CHECK(!qm_arena || qm_elems == lr_elems, -2, "hrn_collate_device: the QM arena must have the LR arena's size (%lld elements, got %lld)",
              (long long)lr_elems, (long long)qm_elems);
    HRN_CHECK(((uintptr_t)lr_arena | (uintptr_t)hr_arena) % 8 == 0 && ((uintptr_t)sm_arena | (uintptr_t)qm_arena) % 4 == 0, -2,
              "hrn_collate_device: arenas must be 8-byte (uint16) / 4-byte (uint8) aligned");
    HRN_CHECK((uintptr_t)codes % 4 == 0, -2, "hrn_collate_device: codes must be 4-byte aligned");
    const bool vec = S % 4 == 0 && ((uintptr_t)lrs | (uintptr_t)hrs | (uintptr_t)maps | (uintptr_t)lr_masks) % 16 == 0;
    if (lr_masks)                                        // the instances with masks live in a translation unit of their own
        return hrn_launch_collate_masks(vec, lr_arena, lr_elems, hr_arena, hr_elems, sm_arena, sm_elems, qm_arena, plan, codes, B, min_L, S, scale,
                                        lrs, alphas, hrs, maps, lr_masks, (hipStream_t)stream);
    const int pieces = scale * scale;
    const dim3 grid((unsigned)(min_L + pieces + (hrs ? pieces : 0)), (unsigned)B);
    auto kernel = vec ? (codes ? collate_kernel<true, true> : collate_kernel<true, false>)
                      : (codes ? collate_kernel<false, true> : collate_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, lr_arena, (long long)lr_elems, hr_arena, (long long)hr_elems,
                       sm_arena, (long long)sm_elems, (const long long*)plan, (const int*)codes, min_L, S, scale, lrs, alphas, hrs, maps);
    HRN_LAUNCH_CHECK();
    return 0;
}

extern "C" int hrn_collate_device_a(const uint16_t* lr_arena, int64_t lr_elems, const uint16_t* hr_arena, int64_t hr_elems,
                                    const uint8_t* sm_arena, int64_t sm_elems, const int64_t* plan, int B, int min_L, int S, int scale,
                                    float* lrs, float* alphas, float* hrs, float* maps, const int32_t* codes, void* stream) {
    return hrn_collate_device_m(lr_arena, lr_elems, hr_arena, hr_elems, sm_arena, sm_elems, nullptr, 0, plan, B, min_L, S, scale, lrs, alphas, hrs,
                                maps, nullptr, codes, stream);
}
